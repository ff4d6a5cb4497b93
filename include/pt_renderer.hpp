// pt_renderer.hpp -- header-only C++ shim with the method set and call order of the reference's abstract
// Renderer (reference: src/renderer.h:30-48), implemented on the C ABI of libptmi.so (pt_api.h).
//
// Vulkan does not exist on the target, so the Vulkan handle parameters of the reference signature are dropped
// here; INTEGRATION.md shows the variant that keeps the reference's exact signatures inside its own tree.
// Methods are `void` like the reference's; failures are reported through lastError() / ok() (the reference
// itself asserts or ignores VkResults, src/rtx_pipeline.cpp:209,237).
#pragma once
#include <string>
#include "pt_api.h"

namespace ptmi {

struct Extent2D {
  uint32_t width, height;
};

class Renderer {  // src/renderer.h:30-48
public:
  virtual ~Renderer() = default;
  virtual void              setup(int deviceOrdinal)                                          = 0;  // (VkDevice, VkPhysicalDevice, familyIndex, allocator)
  virtual void              destroy()                                                         = 0;
  virtual void              run(const Extent2D& size)                                         = 0;  // (cmdBuf, size, profiler, descSets)
  virtual void              create(const Extent2D& size, const pt_SceneDesc* scene = nullptr) = 0;  // (size, layouts, Scene*)
  virtual const std::string name()                                                            = 0;
  void                      setPushContants(const pt_RtxState& state) { m_state = state; }          // (sic) src/renderer.h:44
  pt_RtxState               m_state{};
};

class HipPathTracer : public Renderer {
public:
  ~HipPathTracer() override { destroy(); }
  void setup(int deviceOrdinal) override
  {
    if(!m_ctx)
      check(pt_create(deviceOrdinal, &m_ctx));
  }
  void destroy() override
  {
    if(m_ctx)
      pt_destroy(m_ctx);
    m_ctx = nullptr;
  }
  void create(const Extent2D& size, const pt_SceneDesc* scene = nullptr) override
  {
    if(scene && check(pt_set_scene(m_ctx, scene)))
      check(pt_build_accel(m_ctx));
    check(pt_resize(m_ctx, int(size.width), int(size.height)));
  }
  void run(const Extent2D& size) override
  {
    m_state.size[0] = int(size.width);
    m_state.size[1] = int(size.height);
    check(pt_render_frame(m_ctx, &m_state));
  }
  const std::string name() override { return pt_renderer_name(); }

  // what the reference hands over through descriptor sets 2 and 3
  void setCamera(const pt_SceneCamera& c) { check(pt_set_camera(m_ctx, &c)); }
  // PT_VARIANT_RAYQUERY (the reference's RayQuery renderer, default) or PT_VARIANT_RTX (its RtxPipeline)
  void setVariant(int variant) { check(pt_set_variant(m_ctx, variant)); }
  void setSunAndSky(const pt_SunAndSky& s) { check(pt_set_sunsky(m_ctx, &s)); }
  void setEnvironment(const float* rgba32f, int w, int h, float* integral, float* average) { check(pt_set_env(m_ctx, rgba32f, w, h, integral, average)); }
  // HdrSampling::loadEnvironment (src/hdr_sampling.cpp:56-99) for a Radiance .hdr file: decode (the stbi_loadf of :64), upload, alias table
  bool loadEnvironment(const char* hdrPath, float* integral, float* average)
  {
    float* px = nullptr;
    int    w = 0, h = 0;
    char   err[256] = {0};
    if(pt_hdr_load(hdrPath, &px, &w, &h, err, sizeof(err)) != PT_OK)
    {
      m_error = err;
      return false;
    }
    const bool ok = check(pt_set_env(m_ctx, px, w, h, integral, average));
    pt_hdr_free(px);
    return ok;
  }
  // Scene::load for a .gltf / .glb file (src/scene.cpp:56-118): imports, uploads, builds the acceleration structure and sets the
  // file's first camera (or a fit to the bounding box) for the given aspect ratio.  Returns false and keeps lastError() on failure.
  bool loadGltf(const char* path, float aspect)
  {
    pt_GltfScene* sc = nullptr;
    char          msg[512];
    if(pt_gltf_load(path, &sc, msg, sizeof(msg)) != PT_OK)
    {
      m_status = PT_ERR_INVALID;
      m_error  = msg;
      return false;
    }
    const pt_SceneDesc* d  = pt_gltf_desc(sc);
    bool                ok = check(pt_set_scene(m_ctx, d)) && check(pt_build_accel(m_ctx));
    float               eye[3], center[3], up[3], fov;
    pt_SceneCamera      cam{};
    if(ok && pt_gltf_camera(sc, eye, center, up, &fov) == PT_OK && check(pt_camera_lookat(eye, center, up, fov, aspect, &cam)))
    {
      cam.nbLights = int(d->numLights);
      ok           = check(pt_set_camera(m_ctx, &cam));
    }
    pt_gltf_free(sc);  // pt_set_scene copied everything
    return ok;
  }
  // SampleExample::screenPicking (src/sample_example.cpp:468-511)
  bool pick(float x, float y, const pt_SceneCamera& cam, pt_PickResult* out) { return check(pt_pick(m_ctx, x, y, cam.viewInverse, cam.projInverse, out)); }
  // many screenPicking-style rays at once (and the path tracer's own closest-hit / shadow rays): pt_trace_rays on host arrays ...
  bool traceRays(int kind, uint64_t n, const pt_Ray* rays, pt_RayHit* hits, uint32_t hitsPerRay = 1) { return check(pt_trace_rays(m_ctx, kind, 0u, n, rays, hits, hitsPerRay)); }
  // ... and on 16-byte aligned device memory of the context's GPU, in place
  bool traceRaysDevice(int kind, uint64_t n, const pt_Ray* dRays, pt_RayHit* dHits, uint32_t hitsPerRay = 1) { return check(pt_trace_rays(m_ctx, kind, PT_RAYS_DEVICE, n, dRays, dHits, hitsPerRay)); }
  // the radiance along a caller's own rays (PathTrace of shaders/pathtrace.glsl under the sample loop of pathtrace.comp, without its camera and
  // image): pt_trace_paths on host arrays, and on 16-byte aligned device memory of the context's GPU
  bool tracePaths(const pt_RtxState& state, uint64_t n, const pt_Ray* rays, pt_PathResult* results) { return check(pt_trace_paths(m_ctx, &state, 0u, n, rays, results)); }
  bool tracePathsDevice(const pt_RtxState& state, uint64_t n, const pt_Ray* dRays, pt_PathResult* dResults) { return check(pt_trace_paths(m_ctx, &state, PT_RAYS_DEVICE, n, dRays, dResults)); }
  // the light arriving at the caller's points (no counterpart in the reference, which has no baker): pt_gather -- irradiance from cosine-distributed
  // paths about each point's normal, spherical-harmonic probes from uniformly distributed ones -- on host arrays, and on 16-byte aligned device memory
  bool gatherIrradiance(const pt_RtxState& state, uint64_t n, const pt_GatherPoint* points, pt_GatherResult* results) { return check(pt_gather(m_ctx, &state, PT_GATHER_HEMISPHERE, 0u, n, points, results)); }
  bool gatherProbes(const pt_RtxState& state, uint64_t n, const pt_GatherPoint* points, pt_ProbeResult* results) { return check(pt_gather(m_ctx, &state, PT_GATHER_SPHERE, 0u, n, points, results)); }
  bool gatherDevice(const pt_RtxState& state, uint32_t kind, uint64_t n, const pt_GatherPoint* dPoints, void* dResults) { return check(pt_gather(m_ctx, &state, kind, PT_RAYS_DEVICE, n, dPoints, dResults)); }
  void readAccum(float* rgba32f) { check(pt_read_accum(m_ctx, rgba32f)); }
  void writeAccum(const float* rgba32f) { check(pt_write_accum(m_ctx, rgba32f)); }  // checkpoint restore
  void useAnyHit(bool enable) { check(pt_use_any_hit(m_ctx, enable ? 1 : 0)); }  // RtxPipeline::useAnyHit
  void setAccelMode(int mode) { check(pt_set_accel_mode(m_ctx, mode)); }  // PT_ACCEL_TWO_LEVEL: AccelStructure's BLAS per prim-mesh + TLAS (src/accelstruct.cpp:110-162)
  void updateInstances(const pt_Node* nodes, uint32_t n) { check(pt_update_instances(m_ctx, nodes, n)); }  // new node.worldMatrix values: TLAS refit
  // deforming meshes (no reference counterpart): new vertex records for a range of the vertex buffer, then a refit of the built
  // hierarchies that keeps their topology (costAfter / costBefore of the info says when buildAccel is due); nothing walks the structure in between
  void updateVertices(uint32_t first, uint32_t n, const pt_VertexAttributes* vertices) { check(pt_update_vertices(m_ctx, first, n, vertices)); }
  pt_RefitInfo refitAccel()
  {
    pt_RefitInfo info{};
    check(pt_refit_accel(m_ctx, &info));
    return info;
  }
  void tonemap(const pt_Tonemapper& tm, uint8_t* rgba8) { check(pt_tonemap(m_ctx, &tm, rgba8)); }
  // while SampleExample de-scales (m_descaling, src/sample_example.cpp:410-413): viewport of dispW x dispH from the reduced-size render
  void tonemapZoom(const pt_Tonemapper& tm, int dispW, int dispH, uint8_t* rgba8) { check(pt_tonemap_zoom(m_ctx, &tm, dispW, dispH, rgba8)); }
  // the display pass with frames in flight (main.cpp:213 prepareFrame / :261 submitFrame): begin after every frame, end returns the oldest image
  void tonemapBegin(const pt_Tonemapper& tm, int dispW, int dispH) { check(pt_tonemap_begin(m_ctx, &tm, dispW, dispH)); }
  void tonemapEnd(uint8_t* rgba8) { check(pt_tonemap_end(m_ctx, rgba8)); }
  int  tonemapPending() const { return pt_tonemap_pending(m_ctx); }
  // the edge-avoiding a-trous denoiser between the accumulation image and the display pass (no reference counterpart): guide planes from the caller
  // (each NULL or width * height * 4 floats: albedo, normal, depth), the filtered accumulation image, and the display pass of it
  bool setDenoiseGuides(const float* albedo, const float* normal, const float* depth)
  {
    const float* const planes[PT_DENOISE_GUIDES] = {albedo, normal, depth};
    return check(pt_set_denoise_guides(m_ctx, planes));
  }
  // ... or rendered on the device for the current camera (planes: PT_GUIDES_* mask; asynchronous), and read back (each pointer NULL or width * height * 4 floats).
  // (The default missDepth = 1e30 is beyond the temporal stage's domain of about 1e18: misses then carry no history; see temporalAccumulate.)
  bool renderGuides(uint32_t planes = PT_GUIDES_BASECOLOR | PT_GUIDES_NORMAL | PT_GUIDES_DEPTH, float missDepth = 1.0e30f) { return check(pt_render_guides(m_ctx, planes, missDepth)); }
  bool readDenoiseGuides(float* albedo, float* normal, float* depth)
  {
    float* const planes[PT_DENOISE_GUIDES] = {albedo, normal, depth};
    return check(pt_read_denoise_guides(m_ctx, planes));
  }
  bool denoise(const pt_DenoiseParams& p, float* rgba32f) { return check(pt_denoise(m_ctx, &p, rgba32f)); }
  bool tonemapDenoised(const pt_DenoiseParams& p, const pt_Tonemapper& tm, uint8_t* rgba8) { return check(pt_tonemap_denoised(m_ctx, &p, &tm, rgba8)); }
  // temporal reprojection (no reference counterpart): the history across camera moves.  worldToClip in `p` is the CURRENT camera's forward matrix
  // (pt_camera_world_to_clip).  With renderGuides' default missDepth = 1e30 a miss has no history: its squared distance overflows (pt_api.h); pass a
  // miss depth below about 1e18 to carry the sky along under rotation.
  bool temporalAccumulate(const pt_TemporalParams& p, float* rgba32f = nullptr) { return check(pt_temporal_accumulate(m_ctx, &p, rgba32f)); }
  bool temporalReset() { return check(pt_temporal_reset(m_ctx)); }
  bool readTemporalHistory(float* rgba32f, float* length) { return check(pt_read_temporal_history(m_ctx, rgba32f, length)); }
  // ... or for the first surface behind mirrors and clear glass (no reference counterpart): the same planes, and the link plane
  // (width * height words: links | end << 8) read back
  bool renderGuidesChain(const pt_GuideChain& chain, uint32_t planes = PT_GUIDES_BASECOLOR | PT_GUIDES_NORMAL | PT_GUIDES_DEPTH, float missDepth = 1.0e30f)
  {
    return check(pt_render_guides_chain(m_ctx, &chain, planes, missDepth));
  }
  bool readGuideChain(uint32_t* links) { return check(pt_read_guide_chain(m_ctx, links)); }
  // motion of moving instances (no reference counterpart): after updateInstances, renderInstancePlane in place of renderGuides
  // (the same pass; guidePlanes may be 0) and temporalAccumulateMoving in place of temporalAccumulate -- pixels of a node that moved take their point and
  // normal through its motion before they are reprojected.  The plane holds node indices (width * height words; PT_INSTANCE_NONE: nothing hit).
  bool renderInstancePlane(uint32_t guidePlanes = PT_GUIDES_BASECOLOR | PT_GUIDES_NORMAL | PT_GUIDES_DEPTH, float missDepth = 1.0e30f)
  {
    return check(pt_render_instance_plane(m_ctx, guidePlanes, missDepth));
  }
  bool setInstancePlane(const uint32_t* ids) { return check(pt_set_instance_plane(m_ctx, ids)); }
  bool readInstancePlane(uint32_t* ids) { return check(pt_read_instance_plane(m_ctx, ids)); }
  bool temporalAccumulateMoving(const pt_TemporalParams& p, float* rgba32f = nullptr) { return check(pt_temporal_accumulate_moving(m_ctx, &p, rgba32f)); }
  // variance-guided filter of the history (no reference counterpart): with trackMoments(true) temporalAccumulate also keeps the
  // luminance moments, from which svgfVariance estimates a per-pixel variance and svgfHistory / tonemapSvgf filter the history with a luminance stop
  // measured in standard deviations.  A change of trackMoments drops the history.
  bool trackMoments(bool on) { return check(pt_temporal_track_moments(m_ctx, on ? 1 : 0)); }
  bool readTemporalMoments(float* m) { return check(pt_read_temporal_moments(m_ctx, m)); }
  bool svgfVariance(const pt_SvgfParams& p, float* variance) { return check(pt_svgf_variance(m_ctx, &p, variance)); }
  bool svgfHistory(const pt_SvgfParams& p, float* rgba32f, float* variance = nullptr) { return check(pt_svgf_history(m_ctx, &p, rgba32f, variance)); }
  bool tonemapSvgf(const pt_SvgfParams& p, const pt_Tonemapper& tm, uint8_t* rgba8) { return check(pt_tonemap_svgf(m_ctx, &p, &tm, rgba8)); }
  // demodulated history (no reference counterpart): with temporalDemodulate(true) temporalAccumulate[Moving] divide the pixel's
  // own colour by guide plane 0 (the albedo) as they read it -- the history, its moments and the filters work on illumination -- and svgfHistory,
  // tonemapSvgf, denoiseHistory and tonemapHistory multiply their final image by guide plane 0 again.  All of them need guide plane 0 then.  A change
  // drops the history.
  bool temporalDemodulate(bool on) { return check(pt_temporal_demodulate(m_ctx, on ? 1 : 0)); }
  // responsive history (no reference counterpart): with temporalFast(&p) temporalAccumulate[Moving] keep a second, short history
  // (p.maxFast in the place of maxHistory) beside the long one, clamp the long one to the short one's local mean +- p.sigmaScale standard deviations and
  // cut the history length to maxFast where the clamp moved a channel, so that a change of lighting the guides cannot see shows within a few frames.
  // nullptr: off.  Going from off to on or back drops the history; new parameters do not.
  bool temporalFast(const pt_FastParams* p) { return check(pt_temporal_fast(m_ctx, p)); }
  bool readTemporalFast(float* rgba32f, float* length) { return check(pt_read_temporal_fast(m_ctx, rgba32f, length)); }
  bool denoiseHistory(const pt_DenoiseParams& p, float* rgba32f) { return check(pt_denoise_history(m_ctx, &p, rgba32f)); }
  // dp == nullptr: no spatial filter
  bool tonemapHistory(const pt_DenoiseParams* dp, const pt_Tonemapper& tm, uint8_t* rgba8) { return check(pt_tonemap_history(m_ctx, dp, &tm, rgba8)); }

  bool               ok() const { return m_status == PT_OK; }
  int                status() const { return m_status; }
  const std::string& lastError() const { return m_error; }
  pt_context*        context() { return m_ctx; }

private:
  bool check(int rc)
  {
    m_status = rc;
    if(rc != PT_OK)
      m_error = pt_last_error(m_ctx);
    return rc == PT_OK;
  }
  pt_context* m_ctx    = nullptr;
  int         m_status = PT_OK;
  std::string m_error;
};

}  // namespace ptmi
