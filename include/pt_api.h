/*
 * pt_api.h -- C ABI of libptmi.so, the MI355X (gfx950) path-tracing backend that sits where the
 * reference's Vulkan renderers sit (reference: src/renderer.h:30-48; the two implementations it
 * replaces are src/rayquery.cpp:40-109 and src/rtx_pipeline.cpp:45-276).
 *
 * Conventions
 *  - every entry point returns pt_Status (0 == ok, negative == error); the text of the last error
 *    is available from pt_last_error().  Nothing here aborts the process.  (The reference has no
 *    error convention at all: its methods are void and VkResults are asserted,
 *    src/rtx_pipeline.cpp:209,237.)
 *  - a context is externally synchronised: any thread may call, never two at once.
 *  - host arrays passed to pt_set_* are copied before the call returns.
 *  - pt_render_frame is asynchronous on the context's HIP stream; pt_read_accum, pt_tonemap,
 *    pt_get_stats and pt_synchronize wait for it.
 *  - Traversal-stack overflow: a ray whose walk needs more than 64 stack entries drops a subtree, so the image misses geometry.  Once
 *    such an overflow has been counted, every call that hands out results returns PT_ERR_STATE ("BVH traversal stack overflowed ...")
 *    instead of PT_OK: pt_synchronize, pt_read_accum, pt_tonemap, pt_tonemap_zoom, pt_tonemap_end, pt_denoise, pt_tonemap_denoised, pt_read_denoise_guides, pt_pick,
 *    pt_trace_rays, pt_local_shard, pt_gather_shards and pt_get_stats, and pt_tonemap_begin once the overflow is known (it then enqueues nothing).  The state stays
 *    until pt_reset_stats or the next pt_build_accel (a new scene) clears it; images begun before the clear no longer report it.
 *  - there is no CPU fallback: without a gfx950 device pt_create fails with PT_ERR_NO_DEVICE.
 */
#ifndef PT_API_H
#define PT_API_H

#include <stddef.h>
#include <stdint.h>
#include "pt_types.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* libptmi.so is built with -fvisibility=hidden: exactly these entry points are exported */
#endif

typedef struct pt_context pt_context;

typedef enum pt_Status {
  PT_OK            = 0,
  PT_ERR_INVALID   = -1, /* bad argument / inconsistent scene description */
  PT_ERR_NO_DEVICE = -2, /* no HIP device with that ordinal (or not gfx950) */
  PT_ERR_HIP       = -3, /* a HIP runtime call failed; see pt_last_error */
  PT_ERR_STATE     = -4, /* call order violated (e.g. render before build_accel) */
  PT_ERR_OOM       = -5,
  PT_ERR_UNAVAILABLE = -6 /* an optional runtime library is missing (librccl.so for the pt_comm_* / pt_gather_* calls); see pt_comm_last_error */
} pt_Status;


/* ---- lifetime ------------------------------------------------------------------------------ */

/* replaces Renderer::setup(device, physicalDevice, familyIndex, allocator)  [src/renderer.h:33-36,
 * src/rayquery.cpp:40-46]: binds the context to one GPU and creates its stream. */
int pt_create(int device_ordinal, pt_context** out_ctx);

/* replaces Renderer::destroy() [src/renderer.h:37, src/rayquery.cpp:51-58] plus the destroy() of
 * Scene / AccelStructure / HdrSampling / RenderOutput, whose device memory the context owns. */
int pt_destroy(pt_context* ctx);

/* "HIP" -- replaces Renderer::name() [src/renderer.h:43; "RQ" src/rayquery.hpp:51, "Rtx" src/rtx_pipeline.hpp:57] */
const char* pt_renderer_name(void);

const char* pt_last_error(const pt_context* ctx); /* ctx may be NULL: last pt_create error */

/* ---- scene (descriptor set 2 of the reference, shaders/layouts.glsl:42-46) ------------------- */

/* replaces the uploads done by Scene::load [src/scene.cpp:56-118]: createMaterialBuffer :339-382,
 * createLightBuffer :304-333, createTextureImages :488-580, createVertexBuffer :190-274,
 * createInstanceDataBuffer :161-176.  The arrays are the ones those functions upload. */
int pt_set_scene(pt_context* ctx, const pt_SceneDesc* scene);

/* replaces AccelStructure::create [src/accelstruct.cpp:55-65] (BLAS per prim-mesh :110-127, TLAS
 * instance per node with opaque / cull-disable flags :132-162): builds the device LBVH over the
 * world-space triangles of every node. */
int pt_build_accel(pt_context* ctx);

/* Layout of the acceleration structure pt_build_accel creates.  PT_ACCEL_FLAT (default): one hierarchy over the world-space triangles of
 * every node (an instanced mesh is stored once per instance).  PT_ACCEL_TWO_LEVEL: the reference's own shape [src/accelstruct.cpp:110-127
 * createBottomLevelAS: one BLAS per prim-mesh; :132-162 createTopLevelAS: one TLAS instance per node carrying node.worldMatrix] -- every
 * prim-mesh is built once in object space and shared by its instances, the top level holds the instances' world boxes.  Rendered pixels are
 * bit-identical in both modes (the triangle test runs on the same world-space vertices).  Rebuilds if a structure exists. */
int pt_set_accel_mode(pt_context* ctx, int mode);

/* New world matrices for the nodes of the current scene (same count, same primMesh per node), e.g. an animated or edited scene: the
 * counterpart of rebuilding the reference's TLAS from node.worldMatrix [src/accelstruct.cpp:137-161] without touching the BLASes
 * (nvvk::RaytracingBuilderKHR::buildTlas with update = true).  PT_ACCEL_TWO_LEVEL refits: instance boxes + instance hierarchy only.
 * PT_ACCEL_FLAT rebuilds the whole structure.  Frames already handed to pt_render_frame keep the old transforms. */
int pt_update_instances(pt_context* ctx, const pt_Node* nodes, uint32_t num_nodes);

/* ---- deforming meshes (no reference counterpart: the reference builds its acceleration structures once, on load) --------------------------------
 * pt_update_vertices replaces vertices[first_vertex .. first_vertex + num_vertices) of the scene's vertex buffer -- the whole record: position,
 * packed normal and tangent, texcoords, colour -- for skinned characters, cloth, morph targets, an edit, a simulation mesh.  The data is copied before
 * the call returns.  It waits for the frames in flight first: frames already handed to pt_render_frame keep the old geometry.  Indices, prim-mesh
 * ranges, nodes and materials stay as they are; the call may be repeated before a refit.  Like pt_set_scene it refuses nothing of a vertex itself:
 * non-finite positions are accepted (and, as there, left out of the per-mesh coordinate bound).
 * Errors: PT_ERR_STATE before pt_set_scene; PT_ERR_INVALID, with nothing changed, for a null pointer with num_vertices > 0 and for a range that
 * leaves the vertex buffer; num_vertices == 0 is PT_OK.
 * With a structure built the call marks it STALE: until pt_refit_accel or pt_build_accel every call that walks the structure (pt_render_frame,
 * pt_trace_rays, pt_trace_paths, pt_gather, pt_pick, pt_render_guides*, pt_render_instance_plane) returns PT_ERR_STATE with a message that names
 * the pending refit.  pt_use_any_hit, pt_set_accel_mode and pt_update_instances treat a stale structure as built and rebuild it in full, which
 * clears the mark.  Without a structure the call only updates the buffer and pt_build_accel builds from the new vertices.
 *
 * pt_refit_accel brings the structure up to date WITHOUT changing its topology: every child reference of every node, every leaf slot's (instance,
 * primitive), every node count and range -- and so the traversal-stack depth -- stay; the leaf records, any-hit texcoords, leaf boxes, inner boxes,
 * child-order tables, compact nodes and shading lines are made again from the vertices, in two-level mode also the per-mesh coordinate bounds, the
 * merged structure's box and the instance hierarchy (as after pt_update_instances).  Rendered values equal those of a structure built from the same
 * vertices bit for bit (trace contract: results do not depend on the topology); what degrades with the deformation is the speed, see pt_RefitInfo.
 * Synchronous like pt_build_accel; afterwards the context is in the state pt_build_accel leaves.  A structure that is not stale is refitted as
 * well and comes out bit-identical.  PT_ERR_STATE when there is no structure to refit.  out_info may be NULL.
 * After a vertex update the history of the temporal stage belongs to other surfaces: drop it (pt_temporal_reset).
 * (Not provided: topology changes, index or vertex-count changes, an automatic rebuild when the cost ratio grows, motion vectors for deformed
 * surfaces, the refit path for pt_update_instances in flat mode, which keeps rebuilding.) */
int pt_update_vertices(pt_context* ctx, uint32_t first_vertex, uint32_t num_vertices, const pt_VertexAttributes* vertices);
int pt_refit_accel(pt_context* ctx, pt_RefitInfo* out_info);

/* replaces Scene::updateCamera's UBO upload [src/scene.cpp:629-668] */
int pt_set_camera(pt_context* ctx, const pt_SceneCamera* cam);

/* ---- environment (descriptor set 3, shaders/layouts.glsl:48-50) ------------------------------ */

/* replaces HdrSampling::loadEnvironment after stbi_loadf [src/hdr_sampling.cpp:56-99]: uploads the
 * RGBA32F lat-long image (row 0 = +Y pole) and the alias table built by createEnvironmentAccel
 * [:187-248]; returns getIntegral()/getAverage() [src/hdr_sampling.hpp:44-45].  The caller sets
 * fireflyClampThreshold = 4 * integral like src/sample_example.cpp:110. */
int pt_set_env(pt_context* ctx, const float* rgba32f, int width, int height, float* out_integral, float* out_average);

/* replaces stbi_loadf(file, &w, &h, &comp, STBI_rgb_alpha) in HdrSampling::loadEnvironment [src/hdr_sampling.cpp:56-66] for Radiance
 * RGBE files (.hdr): row 0 first, RGBA32F with alpha 1, value = mantissa * 2^(exponent - 136) like stb_image; flat and run-length
 * encoded scanlines.  Host only (no GPU).  The image is malloc'ed: free it with pt_hdr_free (the reference: stbi_image_free), then hand
 * it to pt_set_env.  On failure returns PT_ERR_INVALID and writes a message to `err` (may be NULL). */
int  pt_hdr_load(const char* path, float** out_rgba32f, int* out_width, int* out_height, char* err, size_t err_len);
void pt_hdr_free(float* rgba32f);

/* replaces the SunAndSky UBO update in SampleExample::updateUniformBuffer [src/sample_example.cpp:168-178] */
int pt_set_sunsky(pt_context* ctx, const pt_SunAndSky* ss);

/* ---- output (descriptor set 1) --------------------------------------------------------------- */

/* replaces Renderer::create(size, ...) [src/renderer.h:42] + RenderOutput::update(size)
 * [src/render_output.cpp:88-99]: (re)allocates the RGBA32F accumulation tiles and the path state. */
int pt_resize(pt_context* ctx, int width, int height);

/* Image-tile sharding for multi-GPU runs (no reference counterpart).  Rank r of n
 * renders the PT_TILE x PT_TILE tiles with (tx + ty) % n == r; seeds use the global pixel index so
 * the pixels are bit-identical to a 1-GPU render.  Default (0, 1).  Call before pt_resize. */
int pt_set_shard(pt_context* ctx, int rank, int nranks);

/* Selects which of the reference's two Renderer implementations the frames reproduce (SampleExample::RndMethod,
 * src/sample_example.hpp:136-137).  PT_VARIANT_RAYQUERY (default): the compute / ray-query path [src/rayquery.cpp,
 * shaders/pathtrace.comp].  PT_VARIANT_RTX: the ray-tracing-pipeline path [src/rtx_pipeline.cpp, shaders/pathtrace.rgen +
 * .rchit / .rahit / .rmiss], which differs in two observable ways: the per-pixel seed is tea(y * W + x, frame) without the
 * maxSamples factor (pathtrace.rgen:72 vs pathtrace.comp:97), and the stochastic alpha tests of a SHADOW ray draw from a copy
 * of the path's seed, so they do not advance it (traceray_rtx.glsl:54-55 with pathtrace.rahit:44,112).  Everything else
 * (samplePixel, PathTrace, the BSDFs) is the same pathtrace.glsl. */
/* (enum PT_VARIANT_* lives in pt_types.h) */
int pt_set_variant(pt_context* ctx, int variant);

/* replaces RtxPipeline::useAnyHit(enable) [src/rtx_pipeline.cpp:269-276, GUI: src/sample_gui.cpp:140-148].  enable == 0 removes the
 * any-hit stage: every triangle is treated as opaque (no stochastic alpha test, no random draw), which "can be faster, but the scene must
 * be fully opaque".  Default 1.  Rebuilds the acceleration structure if one exists (the reference re-creates its pipeline). */
int pt_use_any_hit(pt_context* ctx, int enable);

/* replaces Renderer::setPushContants(state) + Renderer::run(cmdBuf, size, profiler, descSets)
 * [src/renderer.h:38-45; src/rayquery.cpp:97-109 -> shaders/pathtrace.comp:87-134]: renders
 * state->maxSamples samples for every local pixel and folds them into the accumulation buffer with
 * the reference's running mean (pathtrace.comp:122-133).  state->size must equal the pt_resize size. */
int pt_render_frame(pt_context* ctx, const pt_RtxState* state);

int pt_synchronize(pt_context* ctx);

/* Reads the linear RGBA32F accumulation image, row-major width*height*4 floats (alpha == 1).
 * With nranks > 1 only locally owned pixels are valid unless pt_scatter_shards was called; the others read as zero. */
int pt_read_accum(pt_context* ctx, float* rgba32f_out);

/* Checkpoint restore (no reference counterpart; SURVEY.md section 5 "Checkpoint / resume": the progressive state of the reference is the
 * accumulation image plus RtxState.frame, src/sample_example.cpp:183-207).  Replaces the accumulation image by a row-major
 * width*height*4 float image previously obtained from pt_read_accum; continuing with frame = N reproduces an uninterrupted run bit for bit
 * (the running mean of pathtrace.comp:122-133 only needs the image and the frame index). */
int pt_write_accum(pt_context* ctx, const float* rgba32f_in);

/* replaces RenderOutput::genMipmap + RenderOutput::run [src/render_output.cpp:174-193 -> shaders/post.frag:98-147]: tonemaps the
 * accumulation image into row-major RGBA8.  Tonemapper.autoExposure bit 0 takes the image average from the 1x1 level of the
 * vkCmdBlitImage(LINEAR) mip chain the reference generates, bit 1 selects toneLocalExposure (post.frag:72-96) on that chain. */
int pt_tonemap(pt_context* ctx, const pt_Tonemapper* tm, uint8_t* rgba8_out);

/* The display pass while the viewer de-scales [src/sample_example.cpp:378,410-413; shaders/post.frag:101]: the reference renders
 * (W / level) x (H / level) pixels into the top-left corner of its W x H offscreen image and magnifies them with Tonemapper.zoom =
 * 1 / level (NEAREST sampler).  Here the context is resized to the reduced size and this call produces the disp_width x disp_height
 * RGBA8 viewport from it (texels of the offscreen image outside the rendered corner count as zero; the reference keeps stale data
 * there).  With disp == accumulation size and zoom == 1 it is pt_tonemap. */
int pt_tonemap_zoom(pt_context* ctx, const pt_Tonemapper* tm, int disp_width, int disp_height, uint8_t* rgba8_out);

/* The display pass without a host stall (the reference's display loop keeps several frames in flight: src/main.cpp:201-264 only waits for a
 * free swapchain image in prepareFrame() :213 and queues the frame with submitFrame() :261 -- the host never waits for the frame it just
 * recorded).
 * pt_tonemap_begin enqueues pt_tonemap_zoom's work behind the frames rendered so far and returns; frames rendered afterwards overlap it (their
 * accumulate step waits until the pass has read the accumulation image).  pt_tonemap_end blocks until the OLDEST image begun is in host memory
 * and copies it to rgba8_out (the size given to its pt_tonemap_begin).  At most PT_DISPLAY_RING (8) images may be pending
 * (PT_ERR_STATE beyond, and for pt_tonemap_end with none pending); pt_tonemap_pending returns how many are.  The images are bit-identical to
 * what pt_tonemap_zoom returns at the same point of the frame sequence.  A traversal-stack overflow in the frames an image shows is reported
 * by its pt_tonemap_end (the image is still copied out and leaves the ring); after that pt_tonemap_begin refuses with PT_ERR_STATE, enqueuing
 * nothing, until pt_reset_stats or pt_build_accel clears the overflow (see the top of this file). */
#define PT_DISPLAY_RING 8
int pt_tonemap_begin(pt_context* ctx, const pt_Tonemapper* tm, int disp_width, int disp_height);
int pt_tonemap_end(pt_context* ctx, uint8_t* rgba8_out);
int pt_tonemap_pending(pt_context* ctx);

/* ---- denoiser (no reference counterpart: the reference displays its accumulation image unfiltered) -------------------------------------------
 * An edge-avoiding a-trous filter (Dammertz et al. 2010) as a stage of its own between the accumulation image and the display pass; DESIGN.md
 * "Denoiser" has the definition, csrc/pt_denoise.h the one fp32 operation sequence host and device share.  The stage reads the row-major image
 * pt_read_accum returns and guide planes the CALLER supplies -- typically frame-0 debug frames (base colour, normal) and pt_trace_rays depths, all
 * obtained through entry points that exist already -- or that pt_render_guides renders on the device in a pass of its own; no render kernel
 * captures anything for it. */

/* No reference counterpart.  Installs the guide planes: planes[j] is NULL (plane j unset) or a row-major image of width * height * 4 floats whose
 * .xyz are read; copied before the call returns.  Guides must be finite (the filter's result is unspecified otherwise; its reads stay in bounds).
 * PT_ERR_STATE before pt_resize; a pt_resize to another size drops every plane, because its size no longer fits.  planes == NULL: PT_ERR_INVALID. */
int pt_set_denoise_guides(pt_context* ctx, const float* const planes[PT_DENOISE_GUIDES]);

/* No reference counterpart.  The image pt_read_accum would return, filtered: row-major width * height * 4 floats, alpha copied.  Synchronous like
 * pt_read_accum: waits for the frames in flight and reports their traversal-stack overflow with PT_ERR_STATE.  Read-only with respect to rendering:
 * the accumulation tiles, the path state, the frame slots and every pt_Stats field stay as they are, and a frame rendered afterwards continues the
 * running mean as if the call had not happened.  PT_ERR_STATE: before pt_resize; PT_DENOISE_DEMODULATE without guide plane 0; nranks > 1 without a
 * gathered image (a filter over the zero-filled tiles of other ranks means nothing).  PT_ERR_INVALID, with nothing launched: null arguments,
 * iterations outside 1 .. 8, sigmaColor negative or NaN, sigmaGuide of an installed plane not positive and finite, a sigma so small that 1 / sigma^2
 * overflows, unknown flag bits. */
int pt_denoise(pt_context* ctx, const pt_DenoiseParams* params, float* rgba32f_out);

/* No reference counterpart.  pt_tonemap (viewport = accumulation size) with the denoised image as level 0 of the offscreen image: the bytes are those
 * of pt_tonemap on a context whose accumulation image was replaced by pt_denoise's output with pt_write_accum.  Synchronous; errors as pt_denoise
 * and pt_tonemap.  (Not provided: the pt_tonemap_begin / pt_tonemap_end form and pt_tonemap_zoom of a denoised image.) */
int pt_tonemap_denoised(pt_context* ctx, const pt_DenoiseParams* params, const pt_Tonemapper* tm, uint8_t* rgba8_out);

/* No reference counterpart.  The guide pass (DESIGN.md "Guide pass", csrc/pt_guides.h): renders the selected guide planes for the current camera at
 * the pt_resize size, on the device, straight into the context's guide planes -- one first-hit pass of a kernel of its own, no render kernel and no
 * host round trip.  Per pixel: the camera ray of the first sample of frame 0 (seed tea(W * y + x, 0), jitter (0.5, 0.5), the two depth-of-field
 * draws), its closest hit under the trace contract (T5: culling, stochastic alpha from the running seed), and there plane 0 = (base colour, 1),
 * plane 1 = ((normal + 1) / 2, 1) -- what a frame-0 debug frame (eBaseColor / eNormal, maxDepth >= 2) accumulates -- and plane 2 = (t, 0, 0, 0);
 * a miss gives (0, 0, 0, 1), (0, 0, 0, 1) and (miss_depth, 0, 0, 0).  A selected plane replaces whatever the caller installed in it; a plane outside
 * the mask stays as it is, installed or unset.  The whole image is rendered whatever pt_set_shard says (the scene is replicated, and the denoiser
 * only runs on a gathered image).  Asynchronous on the context's stream like pt_render_frame: the next synchronising call reports a traversal-stack
 * overflow of its walks.  The accumulation tiles, the path state, the frame slots and every pt_Stats field stay as they are: a frame sequence with
 * calls in between continues bit for bit.  PT_ERR_STATE: before pt_set_scene / pt_build_accel, before pt_set_camera, before pt_resize.
 * PT_ERR_INVALID, with nothing launched: planes == 0, unknown mask bits, miss_depth not finite (guides must be finite). */
#define PT_GUIDES_BASECOLOR 1u /* plane 0 */
#define PT_GUIDES_NORMAL 2u    /* plane 1 */
#define PT_GUIDES_DEPTH 4u     /* plane 2 */
int pt_render_guides(pt_context* ctx, uint32_t planes, float miss_depth);

/* No reference counterpart.  Copies every installed guide plane j whose planes_out[j] is not NULL to it (width * height * 4 floats, row-major), whether
 * pt_set_denoise_guides or pt_render_guides put it there.  Synchronous like pt_read_accum: waits for the work in flight and reports its
 * traversal-stack overflow with PT_ERR_STATE.  PT_ERR_STATE: before pt_resize; a requested plane that is not installed (nothing is copied).
 * planes_out == NULL: PT_ERR_INVALID. */
int pt_read_denoise_guides(pt_context* ctx, float* const planes_out[PT_DENOISE_GUIDES]);

/* ---- temporal reprojection (no reference counterpart: the reference restarts its accumulation on every camera change) ------------------------
 * The temporal half of SVGF as a stage of its own, the companion of the denoiser above: last call's result -- the *history* the context keeps -- is
 * reprojected into the current camera through the depth guide, tested tap by tap against depth and normal, and blended with the accumulation
 * image.  DESIGN.md section 5.3 has the definition, csrc/pt_temporal.h the one fp32 operation sequence host and device share.  Typical use after a
 * camera move: pt_set_camera, pt_render_guides, pt_render_frame (frame 0), pt_temporal_accumulate, pt_tonemap_history.  No render kernel captures
 * anything for it. */

/* No reference counterpart.  One step of the stage: reads the image pt_read_accum would return, guide planes 1 (normal) and 2 (depth) and the camera
 * of pt_set_camera; writes only the history, which becomes the blended image (colour, normal and depth, length), made with params->worldToClip.
 * rgba32f_out (may be NULL): the new history colour, width * height * 4 floats, alpha the accumulation image's.  The first call, and the first after
 * pt_temporal_reset or a pt_resize to another size, has no history: it stores the current image.  Synchronous like pt_denoise: waits for the frames
 * in flight and reports their traversal-stack overflow with PT_ERR_STATE.  The accumulation tiles, the path state, the frame slots, the guide planes
 * and every pt_Stats field stay as they are.  Depths (miss_depth included) must stay below about 1e18: beyond it the squared distance overflows and
 * the pixel simply has no history.  PT_ERR_STATE: before pt_resize; before pt_set_camera; without guide planes 1 and 2 installed (pt_render_guides or
 * pt_set_denoise_guides); nranks > 1 without a gathered image.  PT_ERR_INVALID, with nothing launched and the history untouched: null parameters, a
 * worldToClip entry that is not finite, depthTol not positive and finite, normalDist2 negative or not finite, maxHistory below 1 or not finite, any
 * flag bit.  With pt_temporal_demodulate on: the pixel's own colour is divided by guide plane 0 as it is read, the history and rgba32f_out hold
 * illumination, and guide plane 0 is needed as well (PT_ERR_STATE without it). */
int pt_temporal_accumulate(pt_context* ctx, const pt_TemporalParams* params, float* rgba32f_out);

/* No reference counterpart.  Drops the history (a scene change, a cut): the next pt_temporal_accumulate behaves as a first call.  No error besides a
 * null context. */
int pt_temporal_reset(pt_context* ctx);

/* No reference counterpart.  Copies the history's colour image (width * height * 4 floats) and its length plane (width * height floats) out; either
 * pointer may be NULL; the colour as it is stored -- illumination, if the history was made with pt_temporal_demodulate on.  Synchronous.  PT_ERR_STATE:
 * there is no history. */
int pt_read_temporal_history(pt_context* ctx, float* rgba32f_out, float* length_out);

/* No reference counterpart.  pt_denoise with the history's colour image in place of the accumulation image: the same filter, the current guide planes,
 * the same parameter checks.  Read-only with respect to the history.  PT_ERR_STATE: before pt_resize; there is no history; PT_DENOISE_DEMODULATE
 * without guide plane 0.  PT_ERR_INVALID as pt_denoise.  On a demodulated history (pt_temporal_demodulate) the filter runs on the illumination and the
 * image after the last iteration is multiplied by guide plane 0, once; PT_ERR_STATE then without guide plane 0, and with PT_DENOISE_DEMODULATE (the
 * history is already demodulated). */
int pt_denoise_history(pt_context* ctx, const pt_DenoiseParams* params, float* rgba32f_out);

/* No reference counterpart.  pt_tonemap_denoised with the history's colour image in place of the accumulation image; params == NULL: no spatial
 * filter, and the bytes are those of pt_tonemap on a context whose accumulation image was replaced by the history with pt_write_accum.  Read-only
 * with respect to the history.  Errors as pt_denoise_history (params != NULL) and pt_tonemap; tm or rgba8_out NULL: PT_ERR_INVALID.  (Not provided:
 * pt_tonemap_zoom of the history and a begin / end form.)  On a demodulated history (pt_temporal_demodulate) the image that is shown -- the filtered one,
 * or the history itself for params == NULL -- is multiplied by guide plane 0 first, as pt_denoise_history does, with its refusals. */
int pt_tonemap_history(pt_context* ctx, const pt_DenoiseParams* params, const pt_Tonemapper* tm, uint8_t* rgba8_out);

/* ---- variance-guided filtering of the history (no reference counterpart) -----------------------------------------------------------------------
 * The spatial half of SVGF, which completes the 1 spp display path: while tracking is on, the history also keeps the first two moments of the
 * luminance; from them (where the history is long) or from a 7 x 7 neighbourhood (where it is short) every pixel gets a variance estimate, and the
 * a-trous filter stops at luminance differences measured in standard deviations of it, carrying the variance through its iterations.  DESIGN.md
 * section 5.4 has the definition, csrc/pt_svgf.h the one fp32 operation sequence host and device share.  Typical use: pt_temporal_track_moments(1)
 * once, then per camera move pt_set_camera, pt_render_guides, pt_render_frame (frame 0), pt_temporal_accumulate, pt_tonemap_svgf.  No render
 * kernel captures anything for it, and with tracking off every other entry point behaves bit for bit as it does without this section. */

/* No reference counterpart.  on = 1: pt_temporal_accumulate also writes the moments image (width * height * 2 floats: mean of the luminance, mean of
 * its square, blended exactly as the colour is); on = 0 (the default): it does not.  The history's colour, guide and length images and the returned
 * image are bit for bit the same either way.  A change of the value drops the history as pt_temporal_reset does; the setting survives pt_resize.
 * PT_ERR_INVALID: on is neither 0 nor 1. */
int pt_temporal_track_moments(pt_context* ctx, int on);

/* No reference counterpart.  Copies the history's moments image (width * height * 2 floats) out.  Synchronous.  PT_ERR_STATE: there is no history,
 * or it was made while tracking was off.  m_out == NULL: PT_ERR_INVALID. */
int pt_read_temporal_moments(pt_context* ctx, float* m_out);

/* No reference counterpart.  The initial variance estimate V0 of the history alone (width * height floats, each in [0, FLT_MAX]): m2 - m1^2 where the
 * history is at least params->minTemporal long, else the guide-weighted 7 x 7 estimate scaled by minTemporal / length.  Reads the history and the
 * current guide planes (each installed plane gives a term, none is required).  Synchronous like pt_denoise_history: waits for the frames in flight
 * and reports their traversal-stack overflow with PT_ERR_STATE.  The history, the accumulation tiles, the path state, the frame slots, the guide
 * planes and every pt_Stats field stay as they are.  PT_ERR_STATE: before pt_resize; there is no history; the history was made while tracking was
 * off.  PT_ERR_INVALID, with nothing launched: null arguments, iterations outside 1 .. 8, sigmaLum or lumFloor not positive and finite, minTemporal
 * below 1 or not finite, sigmaGuide of an installed plane not positive and finite or so small that 1 / sigma^2 overflows, any flag bit. */
int pt_svgf_variance(pt_context* ctx, const pt_SvgfParams* params, float* variance_out);

/* No reference counterpart.  The history's colour image after params->iterations iterations of the variance-guided filter (width * height * 4
 * floats, alpha copied), and in variance_out (may be NULL; width * height floats) the variance after the last iteration.  Guides must be finite (the
 * result is unspecified otherwise; reads stay in bounds).  Synchronous; read-only as pt_svgf_variance; errors as pt_svgf_variance.  On a demodulated
 * history (pt_temporal_demodulate) the filter runs on the illumination, whose scale the moments share, and the image after the last iteration is
 * multiplied by guide plane 0, once (PT_ERR_STATE without it, nothing launched); variance_out and pt_svgf_variance stay in demodulated units. */
int pt_svgf_history(pt_context* ctx, const pt_SvgfParams* params, float* rgba32f_out, float* variance_out);

/* No reference counterpart.  pt_tonemap (viewport = accumulation size) with pt_svgf_history's image as level 0 of the offscreen image: the bytes are
 * those of pt_tonemap on a context whose accumulation image was replaced by pt_svgf_history's output with pt_write_accum.  Synchronous; errors as
 * pt_svgf_history and pt_tonemap; tm or rgba8_out NULL: PT_ERR_INVALID.  (Not provided: pt_tonemap_zoom of the filtered history and a begin / end
 * form.)  On a demodulated history that output, and so the bytes, are of the remodulated image. */
int pt_tonemap_svgf(pt_context* ctx, const pt_SvgfParams* params, const pt_Tonemapper* tm, uint8_t* rgba8_out);

/* ---- motion of moving instances (no reference counterpart) -------------------------------------------------------------------------------------
 * pt_temporal_accumulate reprojects as if the world stood still.  After pt_update_instances a surface that slides or turns within itself passes its
 * depth and normal tests at the same pixel and blends the history of another surface point.  These entry points close that: a per-pixel instance
 * plane (the node index of the first hit), the instance transforms the history was made with, kept by the context, and a form of the temporal step
 * that sends the current point and normal of a moved instance back to where they were before it reprojects them.  DESIGN.md section 5.5 has the
 * definition, csrc/pt_motion.h the one fp32 operation sequence host and device share.  Typical use per frame of a moving scene:
 * pt_update_instances, pt_set_camera, pt_render_instance_plane (in place of pt_render_guides), pt_render_frame (frame 0),
 * pt_temporal_accumulate_moving, pt_tonemap_svgf.  No render kernel captures anything for it. */

#define PT_INSTANCE_NONE 0xffffffffu /* instance plane: the pixel's first camera ray hits nothing */

/* No reference counterpart.  pt_render_guides with the instance plane written besides: one first-hit pass of a kernel of its own that writes, per
 * pixel, the node index of the hit of pt_render_guides' ray (what pt_RayHit::instanceID reports for it; PT_INSTANCE_NONE for a miss) into the
 * context's instance plane and the guide planes selected by guide_planes, bit for bit what pt_render_guides writes there.  guide_planes may be 0:
 * only the instance plane.  Asynchronous, side effects and errors as pt_render_guides, except that a mask of 0 is legal. */
int pt_render_instance_plane(pt_context* ctx, uint32_t guide_planes, float miss_depth);

/* No reference counterpart.  Installs a caller-supplied instance plane: width * height words, row-major, copied before the call returns; any bit
 * pattern is legal (a word that is no node index means "no instance").  ids == NULL drops the plane.  PT_ERR_STATE before pt_resize; a pt_resize to
 * another size drops the plane. */
int pt_set_instance_plane(pt_context* ctx, const uint32_t* ids);

/* No reference counterpart.  Copies the instance plane (width * height words) out, whether pt_render_instance_plane or pt_set_instance_plane put it
 * there.  Synchronous like pt_read_denoise_guides.  PT_ERR_STATE: before pt_resize; no plane is installed.  ids_out == NULL: PT_ERR_INVALID. */
int pt_read_instance_plane(pt_context* ctx, uint32_t* ids_out);

/* No reference counterpart.  The chained guide pass (csrc/pt_chain.h): pt_render_guides, but the pixel's camera ray is
 * followed through mirrors and clear glass (pt_GuideChain, pt_types.h) and the selected planes are written for the first surface that is neither:
 * plane 0 the product of the base colours along the chain times the end surface's, plane 1 the end surface's normal, plane 2 the summed length of the
 * chain (the virtual depth, which pt_temporal_accumulate reprojects correctly for a planar mirror).  A chain that leaves the scene after at least one
 * link gives (tint, 1), (0, 0, 0, 1) and (length so far + miss_depth, 0, 0, 0).  With maxLinks == 0, or where nothing is followable, the planes are
 * bit for bit pt_render_guides'.  A kernel of its own; besides the guide planes it writes the context's link plane, one word per pixel:
 * links | end << 8, end = 0 a surface that is not followed, 1 a miss, 2 the link limit, 3 a direction that cannot be followed.  Asynchronous, side
 * effects and errors as pt_render_guides; PT_ERR_INVALID besides, with nothing launched: chain == NULL, maxLinks > PT_GUIDE_CHAIN_MAX_LINKS, a
 * threshold that is negative or not finite, any flag bit. */
int pt_render_guides_chain(pt_context* ctx, const pt_GuideChain* chain, uint32_t planes, float miss_depth);

/* No reference counterpart.  Copies the link plane of the latest pt_render_guides_chain (width * height words, row-major) out.  Synchronous like
 * pt_read_denoise_guides.  PT_ERR_STATE: before pt_resize; no chained pass ran at the current size (a pt_resize to another size drops the plane).
 * links_out == NULL: PT_ERR_INVALID. */
int pt_read_guide_chain(pt_context* ctx, uint32_t* links_out /* W*H, row-major */);

/* No reference counterpart.  pt_temporal_accumulate for a scene whose nodes moved since the history was made (pt_update_instances): a pixel whose
 * instance plane entry names a node whose world matrix changed takes its point and its normal through that node's motion (history transform o inverse
 * of the current one; the inverse transpose for the normal) before the reprojection and the tap tests; every other pixel, and everything that is
 * stored, is pt_temporal_accumulate's.  With no node moved the result is pt_temporal_accumulate's bit for bit.  Both forms leave the instance
 * transforms with the history, and either may follow the other; pt_temporal_track_moments applies to both.  Errors: everything
 * pt_temporal_accumulate refuses, and PT_ERR_STATE without an instance plane, without a scene, and when the history was made with another number of
 * instances than the scene has (the scene was replaced: pt_temporal_reset).  On every refusal nothing is launched and the history is untouched.
 * pt_temporal_demodulate applies as it does to pt_temporal_accumulate.
 * (Not provided: motion of deforming meshes -- after pt_update_vertices the history should be dropped with pt_temporal_reset --, moving lights or
 * materials, motion seen through reflection or refraction.) */
int pt_temporal_accumulate_moving(pt_context* ctx, const pt_TemporalParams* params, float* rgba32f_out);

/* ---- demodulated history (no reference counterpart) ------------------------------------------------------------------------------------------------
 * The temporal step and the filters above work on the product albedo x illumination: on a textured surface they either stop at every texel edge and
 * leave the noise in, or average across texels and erase the texture.  With this setting on the history holds illumination instead -- the pixel's own
 * colour divided by guide plane 0 as the temporal step reads it -- so that the blend, the moments, every variance and the filters see a signal
 * without the texture, and the consumers of the history multiply their final image by guide plane 0 again.  DESIGN.md section 5.6 has the definition,
 * csrc/pt_albedo.h the one fp32 operation sequence host and device share.  Typical use: pt_temporal_demodulate(1) and pt_temporal_track_moments(1)
 * once, then per frame pt_set_camera, pt_render_guides (all three planes), pt_render_frame (frame 0), pt_temporal_accumulate[_moving],
 * pt_tonemap_svgf.  With the setting off every entry point behaves bit for bit as it does without this section. */

/* No reference counterpart.  on = 1: pt_temporal_accumulate and pt_temporal_accumulate_moving read the pixel's own colour c as
 * c.rgb / max(g0.rgb, 0.001) per channel (g0: guide plane 0 at the pixel; a channel that is not finite passes through; alpha untouched -- the
 * division of PT_DENOISE_DEMODULATE), and everything after that read -- the finiteness test (a finite colour whose quotient overflows counts as not
 * finite), the blend, the stored colour, the moments -- is applied to the quotient; the history's taps are read as they are.  They need guide plane 0
 * then: PT_ERR_STATE without it, nothing launched, the history untouched.  rgba32f_out and pt_read_temporal_history return the colour as stored,
 * i.e. illumination.  pt_svgf_history, pt_tonemap_svgf, pt_denoise_history and pt_tonemap_history multiply their final image by
 * max(g0.rgb, 0.001), with the guide plane 0 installed at the time of that call.  on = 0 (the default): none of this.  A change of the value drops
 * the history as pt_temporal_reset does; the setting survives pt_resize and is independent of pt_temporal_track_moments.  PT_ERR_INVALID: on is
 * neither 0 nor 1. */
int pt_temporal_demodulate(pt_context* ctx, int on);

/* ---- responsive history (no reference counterpart) --------------------------------------------------------------------------------------------------
 * The history above follows the camera and moved instances, but not a change the guides cannot see: a moved sun, a changed emitter, another
 * environment map, the shadow of a moved box.  Depth and normal agree there, every tap counts, and with maxHistory = 32 the display still shows 78 % of
 * the old lighting eight frames later.  With this setting on a second, short history is kept beside the long one (ReLAX: "fast history"), the long one
 * is clamped to the short one's local mean +- sigmaScale standard deviations, and the history length is cut to maxFast where the clamp moved a
 * channel ("anti-lag").  DESIGN.md section 5.7 has the definition, csrc/pt_fast.h the one fp32 operation sequence host and device share.  With the
 * setting off every entry point behaves bit for bit as it does without this section. */

/* No reference counterpart.  params != NULL: pt_temporal_accumulate and pt_temporal_accumulate_moving run their step a second time over the fast
 * history (colour and length; the guide image is shared) with maxFast in the place of maxHistory and without moments, then clamp the long history
 * they have just written: per pixel and channel to mean +- sigmaScale * standard deviation of the new fast colour over the (2 radius + 1)^2 window
 * (taps outside the image, with a fast length below 1 or a colour that is not finite are left out; fewer than 2 taps, a pixel whose own length is
 * below 1 or whose colour is not finite, or bounds that are not finite: the pixel is left as it is; alpha and the moments are never touched), and
 * where a channel moved the pixel's history length becomes min(length, maxFast).  rgba32f_out, pt_read_temporal_history and every consumer of the
 * history see the clamped colour and the lowered length.  params == NULL (the default): none of this.  Going from off to on or from on to off drops
 * the history as pt_temporal_reset does; new parameters while the setting stays on do not.  The setting survives pt_resize and is independent of
 * pt_temporal_track_moments and pt_temporal_demodulate (with demodulation on both histories hold illumination).  PT_ERR_INVALID: maxFast not >= 1 or
 * not finite, sigmaScale negative or not finite, radius outside 1 .. 3, a flag bit; the setting and the history stay as they were.
 * (Not provided: a clamp of the moments, a guide-weighted window, begin / end and zoom forms, per-rank histories.) */
int pt_temporal_fast(pt_context* ctx, const pt_FastParams* params /* NULL: off */);

/* Copies the fast history out: colour (RGBA32F, row-major, width * height * 4 floats) and length (width * height floats); either pointer may be NULL.
 * Synchronous.  PT_ERR_STATE: there is no history, or the history was made with pt_temporal_fast off. */
int pt_read_temporal_fast(pt_context* ctx, float* rgba32f_out, float* length_out);

/* Test access to the image the display pass samples: builds the offscreen image of a disp_width x disp_height viewport and its full mip chain exactly
 * as pt_tonemap_zoom does with auto-exposure on, and copies level `level` (RGBA32F, row-major) to rgba32f_out, its extent to *width / *height (each may
 * be NULL).  Returns the number of levels (>= 1), or a negative pt_Result. */
int pt_debug_display_level(pt_context* ctx, int disp_width, int disp_height, int level, float* rgba32f_out, int* width, int* height);

/* Device-side view of the local shard for the RCCL gather: pointer to [maxTilesPerRank][PT_TILE*PT_TILE][4]
 * floats (owned tiles first, in increasing global tile id; padding zero).  Waits for the frames rendered since the last synchronising
 * call and returns PT_ERR_STATE if they overflowed the traversal stack. */
int pt_local_shard(pt_context* ctx, void** device_ptr, size_t* bytes, int* num_local_tiles, int* max_tiles_per_rank);

/* Rank 0 after the gather: gathered_dev holds nranks consecutive shards as returned by
 * pt_local_shard on each rank; places every tile at its global position so that pt_read_accum /
 * pt_tonemap see the full image. */
int pt_scatter_shards(pt_context* ctx, const void* gathered_dev, int nranks);

/* The one collective of the path, natively over RCCL / xGMI (no reference counterpart): every rank's shard goes to `root`
 * in one grouped operation (nranks-1 ncclRecv on the root, one ncclSend per peer: each shard on its own point-to-point link), then the root
 * places the tiles.  librccl.so is opened on first use.
 *   one process per GPU : rank 0 calls pt_comm_get_unique_id and distributes the 128 bytes; every rank pt_comm_init_rank; after rendering
 *                         every rank pt_gather_shards(ctx, comm, 0); rank 0 pt_gather_finish(ctx), then pt_read_accum / pt_tonemap.
 *   one process, N GPUs : pt_comm_init_all; pt_comm_group_begin(); pt_gather_shards(ctx[i], comm[i], 0) for every i; pt_comm_group_end();
 *                         pt_gather_finish(ctx[0]).
 * The communicator's rank / size must equal pt_set_shard's.  Without librccl.so every call of this group returns PT_ERR_UNAVAILABLE
 * (single-GPU hosts never need the library; libptmi.so is built without the RCCL headers).  Only the root allocates the gather buffer;
 * pt_gather_finish on a context that did not enqueue a gather as root returns PT_ERR_STATE.  A rank whose frames overflowed the traversal
 * stack still takes part in the collective (leaving it would stall the peers) and then returns PT_ERR_STATE from pt_gather_shards. */
typedef struct pt_comm pt_comm;
#define PT_COMM_ID_BYTES 128
int pt_comm_get_unique_id(unsigned char id_out[PT_COMM_ID_BYTES]);
int pt_comm_init_rank(int nranks, const unsigned char id[PT_COMM_ID_BYTES], int rank, int device_ordinal, pt_comm** out_comm);
int pt_comm_init_all(int ndev, const int* device_ordinals, pt_comm** out_comms);
int pt_comm_destroy(pt_comm* comm);
/* ranks of the communicator as RCCL reports them (ncclCommCount): what a launcher prints to show that N processes really met */
int pt_comm_count(pt_comm* comm, int* out_nranks);
/* ncclGetVersion of the RCCL that was opened (e.g. 22707), 0 when the library does not say; a preflight of a multi-GPU run prints it */
int pt_comm_version(int* out_version);
/* why the last pt_comm_* call of this thread's process failed (e.g. "librccl.so not found: ..."); never NULL */
const char* pt_comm_last_error(void);
int pt_comm_group_begin(void);
int pt_comm_group_end(void);
int pt_gather_shards(pt_context* ctx, pt_comm* comm, int root);
int pt_gather_finish(pt_context* ctx);

/* ---- measurement ----------------------------------------------------------------------------- */

/* enable != 0: bracket every kernel with HIP events on the render stream and accumulate per-stage
 * milliseconds into pt_Stats (replaces the nvvk::ProfilerVK sections "Render"/"Tonemap",
 * src/sample_example.cpp:404, src/main.cpp:212-257). */
int pt_set_profiling(pt_context* ctx, int enable);
int pt_get_stats(pt_context* ctx, pt_Stats* out);
int pt_reset_stats(pt_context* ctx);

/* ---- host-side helpers restating the reference's scene packing -------------------------------- */

/* shaders/compress.glsl:111-139 (host flavour used at src/scene.cpp:224-225) */
uint32_t pt_compress_unit_vec(const float v[3]);

/* src/scene.cpp:219-242: positions[3n], normals[3n], tangents[4n] (w = handedness), uvs[2n],
 * colors[4n] (float 0..1) -> VertexAttributes[n] */
int pt_pack_vertices(uint32_t n, const float* positions, const float* normals, const float* tangents,
                     const float* uvs, const float* colors, pt_VertexAttributes* out);

/* src/scene.cpp:629-640 with glm::lookAt / perspectiveRH_ZO(fov, aspect, 0.001, 1e5), proj[1][1] *= -1 */
int pt_camera_lookat(const float eye[3], const float center[3], const float up[3], float fov_degrees,
                     float aspect, pt_SceneCamera* out);

/* No reference counterpart (the reference never needs the forward matrix).  out16 = proj * view, column-major, world -> clip, from the same
 * double-precision view and proj whose inverses pt_camera_lookat returns: what pt_TemporalParams::worldToClip takes for a camera set up with
 * pt_camera_lookat (callers with matrices of their own pass their own product).  PT_ERR_INVALID: null pointers, aspect <= 0, eye == center. */
int pt_camera_world_to_clip(const float eye[3], const float center[3], const float up[3], float fov_degrees, float aspect, float out16[16]);

/* src/hdr_sampling.cpp:107-248 on the host; pt_set_env calls this internally. */
int pt_build_env_accel(const float* rgba32f, int width, int height, pt_EnvAccel* out_accel, float* out_integral,
                       float* out_average);

/* src/scene.cpp:447-482,561-571: glTF sampler codes -> filter / wrap enums of pt_TextureDesc
 * (has_sampler == 0: LINEAR / REPEAT; unknown filter code: NEAREST; unknown wrap: REPEAT). */
int pt_sampler_from_gltf(int has_sampler, int gltf_mag, int gltf_min, int gltf_wrapS, int gltf_wrapT, pt_TextureDesc* io);

/* replaces the ray picker of SampleExample::screenPicking [src/sample_example.cpp:468-511 -> nvvk::RayPickerKHR]: shoots one ray through
 * the normalised window position (pick_x, pick_y in [0,1], origin top-left like the reference's cursor position) with the given inverse view
 * and inverse projection matrices (column-major, as in pt_SceneCamera) and returns the nearest triangle -- every triangle counts, without
 * face culling or alpha test, like the picker's flag-less traceRayEXT.  Synchronous: waits for every frame in flight, then reports a
 * traversal-stack overflow of those frames or of its own ray with PT_ERR_STATE. */
int pt_pick(pt_context* ctx, float pick_x, float pick_y, const float view_inverse[16], const float proj_inverse[16], pt_PickResult* out);

/* Batched ray queries against the scene's acceleration structure (no reference counterpart beyond screenPicking: what a caller does with a
 * renderer's scene besides rendering -- visibility and ambient-occlusion baking, light-map sample placement, many picks at once, line-of-sight
 * tests, collision probes).  Traces rays[0 .. n) and writes hits_per_ray results per ray to hits[i * hits_per_ray ..].  Each kind is one piece of
 * the trace contract:
 *   PT_RAYS_CLOSEST    the path tracer's closest-hit ray (T5): face culling by the instance flags, opaque candidates commit, non-opaque ones
 *                      draw in key order from `seed`; `seed` out is the state after the draws.  Unbounded like traceray_rq.glsl's ClosestHit:
 *                      tmax is IGNORED (a caller who wants a bound compares t).
 *   PT_RAYS_OCCLUDED   the shadow ray (T6), bounded by tmax: PT_RAY_HIT means in shadow, no hit field is filled.  `seed` follows the context's
 *                      variant: under PT_VARIANT_RTX it comes back untouched.
 *   PT_RAYS_NEAREST    pt_pick's query: every triangle counts (no culling, no alpha), the nearest key inside (0, tmax).
 *   PT_RAYS_CANDIDATES the first hits_per_ray (1 .. PT_RAYS_MAX_HITS) candidates inside (0, tmax) in key order (t, world triangle index), with
 *                      culling and without alpha; unused entries are misses.  Every other kind requires hits_per_ray == 1.
 * A miss is t = u = v = 0, instanceID = 0xffffffff, primitiveID = instanceCustomIndex = -1; ids mean what they mean in pt_PickResult.  With
 * pt_use_any_hit(0) every triangle is opaque, so no kind draws.  A ray with a non-finite origin or direction component, a zero direction or (bounded
 * kinds) a NaN tmax is not walked: its results are misses with PT_RAY_INVALID set and `seed` unchanged.  tmax <= 0 is an empty range, a plain miss.
 * flags: PT_RAYS_DEVICE -- rays and hits are device pointers on the context's GPU, 16-byte aligned, read and written in place.  Without it they
 * are host arrays, staged in chunks of PT_QUERY_CHUNK records through two device buffers the context allocates on first use.
 * Needs pt_set_scene and pt_build_accel (PT_ERR_STATE before), no pt_resize.  Synchronous like pt_pick: waits for the frames in flight, runs on
 * the context's stream and reports a traversal-stack overflow of those frames or of its own rays with PT_ERR_STATE.  n == 0: PT_OK, nothing is
 * launched.  Null pointers with n > 0, an unknown kind or flag bit, a bad hits_per_ray or a misaligned device pointer: PT_ERR_INVALID, nothing is
 * launched.  A query touches neither the accumulation image, the path state, the frame slots nor any pt_Stats field. */
int pt_trace_rays(pt_context* ctx, int kind, uint32_t flags, uint64_t n, const pt_Ray* rays, pt_RayHit* hits, uint32_t hits_per_ray);

/* Path queries: the radiance along a caller's own rays (stands in for PathTrace of shaders/pathtrace.glsl, called from the sample loop of
 * shaders/pathtrace.comp:97-105, without that shader's pinhole camera and image: light-map and irradiance-probe baking, panoramas, fisheye,
 * orthographic and stereo views, re-sampling chosen pixels, the radiance along one ray from a surface point).  Defined in DESIGN.md section 3.2.
 * Per ray: seed = ray.seed; for each of state->maxSamples samples a path starts on the SAME ray (origin, direction; tmax is ignored, the first ray is
 * unbounded like PT_RAYS_CLOSEST) and runs the frames' path loop to state->maxDepth -- emission, direct light with MIS, both BSDFs, Russian
 * roulette -- on the stream that continues from the previous sample; its radiance is clamped as the frames clamp it (fireflyClampThreshold) and
 * summed in sample order; radiance = sum / maxSamples.  (A frame draws a new camera ray per sample; a caller who wants that changes the ray between
 * one-sample calls.)  One sample on the camera ray of a pixel of frame 0 with that pixel's seed is that pixel of frame 0, bit for bit.
 * state: maxDepth (0 .. PT_MAX_DEPTH), maxSamples (1 .. PT_PATHS_MAX_SAMPLES), fireflyClampThreshold, hdrMultiplier, pbrMode (0 / 1) and
 * debugging_mode (every mode but PT_DEBUG_HEATMAP, which needs a frame's clocks) are read; frame, size and the heat-map bounds are ignored.
 * Invalid rays (pt_trace_rays' rule without tmax): radiance 0, firstT 0, seed unchanged, closestRays 0, status PT_RAY_INVALID; not walked.
 * flags: PT_RAYS_DEVICE as for pt_trace_rays (16-byte aligned device arrays, in place); host arrays are staged through the same two buffers.
 * Needs what pt_render_frame needs of the scene side -- pt_set_scene, pt_build_accel, an environment or sun & sky, pt_set_camera (only its nbLights
 * is read) -- else PT_ERR_STATE; no pt_resize.  Synchronous like pt_trace_rays: waits for the frames in flight, runs on the context's stream,
 * reports a traversal-stack overflow with PT_ERR_STATE.  n == 0: PT_OK.  Null pointers with n > 0, an unknown flag bit, a misaligned device
 * pointer or a state outside the ranges above: PT_ERR_INVALID, nothing is launched.  A path query touches neither the accumulation image, the
 * path state, the frame slots nor any pt_Stats field: frames before and after it come out as if it had not happened. */
int pt_trace_paths(pt_context* ctx, const pt_RtxState* state, uint32_t flags, uint64_t n, const pt_Ray* rays, pt_PathResult* results);

/* Gather queries: the light that arrives at a caller's points (light-map texels, irradiance probes).  The reference has no baker; every sample is
 * PathTrace of shaders/pathtrace.glsl along a direction drawn AT the point -- for PT_GATHER_HEMISPHERE by the BSDF's own cosine sampler
 * (CosineSampleHemisphere of shaders/pbr_disney.glsl in the frame of shaders/common.glsl:80-92 about the point's normal, from the origin
 * OffsetRay gives), for PT_GATHER_SPHERE uniformly over the sphere from the position itself.  Defined in DESIGN.md section 3.3.
 * Per point: seed = point.seed; each of state->maxSamples samples draws two numbers for its direction, then runs pt_trace_paths' path on that ray
 * with the stream that continues from the draws; the radiance is clamped per sample and reduced in sample order:
 *   PT_GATHER_HEMISPHERE  results is pt_GatherResult[n]: irradiance = pi * sum / maxSamples (the pdf is cos / pi, so the cosine cancels)
 *   PT_GATHER_SPHERE      results is pt_ProbeResult[n]:  sh[k] = 4 pi * sum(radiance * Y_k(direction)) / maxSamples, nine real basis functions
 * hitFraction: the samples whose first ray hit geometry / maxSamples.  An invalid point (a non-finite position component; HEMISPHERE also a
 * non-finite or zero normal, or one whose unit vector is not finite and non-zero in fp32: a squared length that under- or overflows) is not walked: numerics 0, seed unchanged, status PT_RAY_INVALID.
 * state, flags (PT_RAYS_DEVICE: 16-byte aligned device arrays, in place; else host arrays staged through the query buffers: PT_QUERY_CHUNK points a
 * piece for HEMISPHERE, PT_QUERY_CHUNK / 4 for SPHERE), what the call needs, its refusals and its synchronisation are pt_trace_paths'.  A kind
 * other than the two: PT_ERR_INVALID.  n == 0: PT_OK.  A gather touches neither the accumulation image, the path state, the frame slots nor any
 * pt_Stats field. */
int pt_gather(pt_context* ctx, const pt_RtxState* state, uint32_t kind, uint32_t flags, uint64_t n, const pt_GatherPoint* points, void* results);

/* Measures, on this device, the two ceilings the measurement contract prices kernels against (no reference counterpart): VALU issue
 * (independent wave64 v_fma_f32 at 8 waves per SIMD on every CU, wave-instructions per second) and HBM streaming (float4 copy and
 * read-only over 1 GiB buffers, bytes per second).  Synchronous, a few tens of milliseconds. */
int pt_measure_peaks(pt_context* ctx, pt_Peaks* out);

/* Evaluates one function of the fp32 transcendental contract (include/pt_fpmath.h; enum PT_FN_* in pt_types.h) on the device for n
 * arguments (b is the second argument of atan2(a, b) / pow(a, b), otherwise ignored and may be NULL).  No reference counterpart: GLSL
 * leaves these functions' accuracy to the driver; the contract fixes one IEEE operation sequence and this entry point lets a test hold
 * the gfx950 evaluation bit for bit to the host evaluation of the same header.  Synchronous. */
int pt_fpmath_eval(pt_context* ctx, int fn, uint64_t n, const float* a, const float* b, float* out);

/* ---- glTF import (host only, no GPU) ------------------------------------------------------------------------------------
 * replaces Scene::load -> loadGltfScene (tinygltf) + nvh::GltfScene::importMaterials / importDrawableNodes + the create*Buffer
 * packing [src/scene.cpp:56-155, 190-382, 488-580] for .gltf and .glb files: the result is the flat pt_SceneDesc pt_set_scene
 * takes (textures are (sampler, image) pairs decoded to RGBA8; PNG and Huffman-coded JPEG, sequential or progressive), plus the first camera of the file or a
 * fit to the bounding box [src/scene.cpp:281-298].  The scene owns every array the description points to until pt_gltf_free.
 * On failure returns PT_ERR_INVALID and writes a message to `err` (may be NULL). */
typedef struct pt_GltfScene pt_GltfScene;
int                 pt_gltf_load(const char* path, pt_GltfScene** out_scene, char* err, size_t err_len);
const pt_SceneDesc* pt_gltf_desc(const pt_GltfScene* scene);
int                 pt_gltf_camera(const pt_GltfScene* scene, float eye[3], float center[3], float up[3], float* fov_degrees);
int                 pt_gltf_bounds(const pt_GltfScene* scene, float bbox_min[3], float bbox_max[3]);
void                pt_gltf_free(pt_GltfScene* scene);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* PT_API_H */
