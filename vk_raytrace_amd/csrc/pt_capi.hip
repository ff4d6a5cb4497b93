// C ABI of libptmi.so (include/pt_api.h): context, device memory, call sequencing of scene upload, frames, read-back and display.
// Host code only: the kernels are pt_render.hip's.  The acceleration-structure calls are pt_capi_accel.hip, the host-side scene
// records pt_scene_records.cpp, calibration and test kernels pt_debug.hip; pt_context.h is what they share.
// Mirrors the division of labour of the reference's host classes -- Scene (src/scene.cpp), AccelStructure
// (src/accelstruct.cpp), HdrSampling (src/hdr_sampling.cpp), RenderOutput (src/render_output.cpp) and the
// Renderer implementations (src/rayquery.cpp, src/rtx_pipeline.cpp) -- behind one opaque pt_context.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include "pt_context.h"
#include "pt_scene_records.h"
#include "pt_stage.h"  // stages_release

static std::string g_createError;

int dev_alloc(pt_context* c, DevBuf& b, size_t bytes)
{
  if(b.p && b.bytes >= bytes && b.bytes <= bytes * 2 + 4096)
    return PT_OK;
  dev_free(b);
  if(bytes == 0)
    bytes = 16;
  HIP_TRY(c, hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  return PT_OK;
}
bool dev_alloc_quiet(DevBuf& b, size_t bytes)
{
  if(b.p && b.bytes >= bytes && b.bytes <= bytes * 2 + 4096)
    return true;
  dev_free(b);
  if(bytes == 0)
    bytes = 16;
  if(hipMalloc(&b.p, bytes) != hipSuccess)
  {
    b.p = nullptr;
    return false;
  }
  b.bytes = bytes;
  return true;
}
void dev_free(DevBuf& b)
{
  if(b.p)
    (void)hipFree(b.p);
  b.p     = nullptr;
  b.bytes = 0;
}
int upload(pt_context* c, DevBuf& b, const void* src, size_t bytes)
{
  int rc = dev_alloc(c, b, bytes);
  if(rc != PT_OK)
    return rc;
  if(bytes)
    HIP_TRY(c, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
  return PT_OK;
}

static inline int slot_total(const pt_context* c) { return c->inflight + c->displaySlots; }
static inline pt_context::FrameSlot& slot_at(pt_context* c, int k) { return c->slots[k < c->inflight ? k : c->inflightMax + (k - c->inflight)]; }

// ---- frame slots -------------------------------------------------------------------------------------------
using FrameSlot = pt_context::FrameSlot;
size_t FrameSlot::bytes_held()
{
  size_t held = 0;
  each_path_buffer([&](DevBuf& b, size_t) { held += b.bytes; });
  return held;
}
bool FrameSlot::alloc(size_t paths)
{
  bool ok = true;
  each_path_buffer([&](DevBuf& b, size_t perPath) { ok = ok && dev_alloc_quiet(b, perPath * paths); });
  return ok && dev_alloc_quiet(dCounts, sizeof(uint32_t) * CNT_STRIDE * (PT_MAX_DEPTH + 2)) && dev_alloc_quiet(dCountsDone, sizeof(uint32_t) * CNT_STRIDE * (PT_MAX_DEPTH + 2));
}
hipError_t FrameSlot::clear_counts()
{
  const hipError_t e = hipMemset(dCounts.p, 0, dCounts.bytes);
  return e != hipSuccess ? e : hipMemset(dCountsDone.p, 0, dCountsDone.bytes);
}
void FrameSlot::release_paths()
{
  each_path_buffer([](DevBuf& b, size_t) { dev_free(b); });
}
void FrameSlot::bind(float4* frame, uint32_t* slotTile, Counters* counters)
{
  PathState& ps = rb.ps;
  ps.rayO.p = (float4*)dState[0].p; ps.rayD.p = (float4*)dState[1].p; ps.thr.p = (float4*)dState[2].p; ps.rad.p = (float4*)dState[3].p;
  ps.absorb.p = (float4*)dState[4].p; ps.neeDir.p = (float4*)dState[5].p; ps.neeRad.p = (float4*)dState[6].p; ps.hit.p = (float4*)dState[7].p;
  ps.sum.p = (float4*)dState[8].p;
  rb.queueA     = (uint32_t*)dQueue[0].p;
  rb.queueB     = (uint32_t*)dQueue[1].p;
  rb.queueS     = (uint32_t*)dQueue[2].p;
  rb.queueX     = (uint32_t*)dQueue[3].p;
  rb.queueX2    = (uint32_t*)dQueue[4].p;
  rb.queueR     = (uint32_t*)dQueue[5].p;
  rb.counts     = (uint32_t*)dCounts.p;
  rb.countsDone = (uint32_t*)dCountsDone.p;
  rb.frame      = frame;
  rb.slotTile   = slotTile;
  rb.counters   = counters;
}

// waits for everything that was launched (frames handed over but not launched yet stay pending)
static hipError_t sync_streams(pt_context* c)
{
  for(int i = 0; i < PT_MAX_INFLIGHT; ++i)
    if(c->slots[i].stream)
    {
      hipError_t e = hipStreamSynchronize(c->slots[i].stream);
      if(e != hipSuccess)
        return e;
    }
  c->lastAccum = nullptr;
  for(int i = 0; i < PT_MAX_INFLIGHT; ++i)
    c->slots[i].launched = false;
  return hipStreamSynchronize(c->stream);
}
hipError_t sync_all(pt_context* c)
{
  return flush_pending(c) != PT_OK ? hipErrorUnknown : sync_streams(c);
}
// After a synchronisation: a traversal that ran out of stack (STACK_LDS + STACK_SPILL entries) dropped a subtree, so the image is wrong --
// every call that hands results to the caller reports it instead of returning PT_OK with missing geometry.
// The rule (include/pt_api.h, "Traversal-stack overflow"): pt_synchronize, pt_read_accum, pt_tonemap / pt_tonemap_zoom, pt_tonemap_end
// (from the counter the display pass copied), pt_pick, pt_local_shard, pt_gather_shards and pt_get_stats return PT_ERR_STATE with this
// message once an overflow has been counted, and so does pt_tonemap_begin once one is known; they keep doing so until the counter is
// cleared -- by pt_reset_stats, or by pt_build_accel, since a new structure makes the old overflows meaningless.
// Callers have synchronised (sync_all): the copies of the counter that pending display images carry have landed and are cleared with it.
void clear_overflow(pt_context* c)
{
  c->overflowSeen       = 0;
  c->renderedSinceCheck = false;
  for(auto& ds : c->display)
    if(ds.overflow)
      *ds.overflow = 0;
}
static int report_overflow(pt_context* c)
{
  return c->fail(PT_ERR_STATE, "BVH traversal stack overflowed %u times (the image is invalid: the acceleration structure is deeper than the traversal stack)",
                 c->overflowSeen);
}
int check_traversal(pt_context* c)
{
  if(c->renderedSinceCheck)
  {
    unsigned int n = 0;
    HIP_TRY(c, hipMemcpy(&n, (const char*)c->dCounters.p + offsetof(Counters, stackOverflow), sizeof(n), hipMemcpyDeviceToHost));
    c->renderedSinceCheck = false;
    c->overflowSeen       = n;
  }
  return c->overflowSeen ? report_overflow(c) : PT_OK;
}

// the instance records as the kernels see them: with useAnyHit(false) every instance carries FORCE_OPAQUE, which is what a hit group
// without an any-hit shader amounts to (src/rtx_pipeline.cpp:186-195)
std::vector<InstanceRec> effective_instances(const pt_context* c)
{
  std::vector<InstanceRec> inst = c->hInstances;
  if(!c->anyHit)
    for(InstanceRec& I : inst)
      I.flags |= TRI_OPAQUE;
  return inst;
}
int upload_instances(pt_context* c)
{
  const std::vector<InstanceRec> inst = effective_instances(c);
  InstanceRec dummy{};
  return upload(c, c->dInstances, inst.empty() ? &dummy : inst.data(), sizeof(InstanceRec) * (inst.empty() ? 1 : inst.size()));
}

void refresh_scene_ptrs(pt_context* c)
{
  DeviceScene& s = c->scene;
  s.vertices     = (const float4*)c->dVertices.p;
  s.indices      = (const uint32_t*)c->dIndices.p;
  s.instances    = (const InstanceRec*)c->dInstances.p;
  s.materials    = (const pt_GltfShadeMaterial*)c->dMaterials.p;
  s.lights       = (const pt_Light*)c->dLights.p;
  s.texRecs      = (const TexRec*)c->dTexRecs.p;
  s.matLines     = (const uint4*)c->dMatLines.p;
  s.texels       = (const uint32_t*)c->dTexels.p;
  s.bvh          = (const BvhNode*)c->dBvh.p;
  s.wide         = (const WideNode*)c->dWide.p;
  s.tris         = (const TriRec*)c->dTris.p;
  s.alphaRecs    = (const AlphaRec*)c->dAlphaRecs.p;
  s.cnodes       = c->haveCNodes ? (const CompactNode*)c->dCNodes.p : nullptr;
  s.ctlas        = c->haveCNodes ? (const CompactNode*)c->dCTlas.p : nullptr;
  s.shadeTris    = c->haveShadeTris ? (const float4*)c->dShadeTris.p : nullptr;
  s.alphaMats    = (const AlphaMat*)c->dAlphaMats.p;
  s.alphaMaps    = (const uint32_t*)c->dAlphaMaps.p;
  s.env          = (const float4*)c->dEnv.p;
  s.envAccel     = (const pt_EnvAccel*)c->dEnvAccel.p;
  s.numTris      = c->numTris;
  s.numInstances = c->numInstances;
  const bool two = c->accelMode == PT_ACCEL_TWO_LEVEL && c->haveAccel && !c->mergedOnly;
  s.tlas         = two ? (const WideNode*)c->dTlas.p : nullptr;
  s.tlasLeaves   = two ? (const TlasLeaf*)c->dTlasLeaves.p : nullptr;
  s.instTriBase  = two ? (const uint32_t*)c->dInstTriBase.p : nullptr;
  s.instBlock    = two ? (const uint32_t*)c->dInstBlock.p : nullptr;
  s.twoLevel     = two ? 1u : 0u;
  s.allOpaque    = 1u;
  for(const InstanceRec& I : c->hInstances)
    if(I.triCount && c->anyHit && !(I.flags & TRI_OPAQUE))
      s.allOpaque = 0u;
}


// ---- stage timers ------------------------------------------------------------------------------------------
void pt_timers_begin(StageTimers* t, hipStream_t s, int stage)
{
  if(!t || !t->enabled)
    return;
  if(t->npend == t->cap)
  {
    size_t ncap = t->cap ? t->cap * 2 : 256;
    auto*  np   = (StageTimers::Pending*)realloc(t->pend, ncap * sizeof(StageTimers::Pending));
    if(!np)
      return;
    for(size_t i = t->cap; i < ncap; ++i)
    {
      (void)hipEventCreate(&np[i].a);
      (void)hipEventCreate(&np[i].b);
    }
    t->pend = np;
    t->cap  = ncap;
  }
  t->pend[t->npend].stage = stage;
  (void)hipEventRecord(t->pend[t->npend].a, s);
}
void pt_timers_end(StageTimers* t, hipStream_t s, int stage)
{
  if(!t || !t->enabled || t->npend >= t->cap)
    return;
  (void)hipEventRecord(t->pend[t->npend].b, s);
  if(stage == 1)
    t->launchesClosest++;
  if(stage == 5)
    t->launchesTail++;
  if(stage == 6)
    t->launchesFused++;
  t->npend++;
  if(t->npend == t->cap && t->cap >= 8192)
    pt_timers_collect(t);  // bound the number of live events
}
void pt_timers_collect(StageTimers* t)
{
  if(!t || !t->npend)
    return;
  (void)hipEventSynchronize(t->pend[t->npend - 1].b);
  for(size_t i = 0; i < t->npend; ++i)
  {
    float ms = 0.f;
    if(hipEventElapsedTime(&ms, t->pend[i].a, t->pend[i].b) == hipSuccess)
      t->ms[t->pend[i].stage] += ms;
  }
  t->npend = 0;
}

extern "C" {

const char* pt_renderer_name(void) { return "HIP"; }

const char* pt_last_error(const pt_context* ctx) { return ctx ? ctx->err.c_str() : g_createError.c_str(); }

// pt_create's failures have no context to carry their message: pt_last_error(NULL) reports it
static int create_fail(int code, const std::string& msg, pt_context* c = nullptr)
{
  g_createError = msg;
  delete c;
  return code;
}
int pt_create(int device_ordinal, pt_context** out_ctx)
{
  if(!out_ctx)
    return PT_ERR_INVALID;
  *out_ctx  = nullptr;
  // frames in flight need one hardware queue each; effective only if the HIP runtime is not initialised yet
  setenv("GPU_MAX_HW_QUEUES", "8", 0);
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if(e != hipSuccess || count <= 0)
    return create_fail(PT_ERR_NO_DEVICE, std::string("no HIP device available: ") + hipGetErrorString(e) + " (libptmi has no CPU fallback)");
  if(device_ordinal < 0 || device_ordinal >= count)
    return create_fail(PT_ERR_NO_DEVICE, "device ordinal " + std::to_string(device_ordinal) + " out of range: " + std::to_string(count) + " HIP device(s) visible to this process");
  hipDeviceProp_t prop;
  if(hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess)
    return create_fail(PT_ERR_HIP, "hipGetDeviceProperties failed");
  if(std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return create_fail(PT_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", libptmi.so is built for gfx950 only");
  if(hipSetDevice(device_ordinal) != hipSuccess)
    return create_fail(PT_ERR_HIP, "hipSetDevice failed");
  // every context has its own knobs (round 6): parsed key by key, defaults otherwise; tokens that name no knob are reported once per process
  PtTuning    parsed;
  std::string unknown;
  pt_parse_tuning(getenv("PT_TUNE"), parsed, unknown);
  if(!unknown.empty())
  {
    static std::atomic<bool> warned{false};
    if(!warned.exchange(true))
      fprintf(stderr, "libptmi: PT_TUNE tokens that name no knob (ignored; removed knobs are constants now, see csrc/pt_internal.h PtTuning): %s\n", unknown.c_str());
  }
  pt_context* c = new pt_context();
  c->tune       = parsed;
  c->device     = device_ordinal;
  c->accelMode  = c->tune.accelTwoLevel ? PT_ACCEL_TWO_LEVEL : PT_ACCEL_FLAT;
  if(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
    return create_fail(PT_ERR_HIP, "hipStreamCreate failed", c);
  c->timers.stream = c->stream;
  c->inflight      = c->tune.framesInFlight < 1 ? 1 : (c->tune.framesInFlight > PT_MAX_INFLIGHT ? PT_MAX_INFLIGHT : c->tune.framesInFlight);
  c->inflightMax = c->inflight;
  c->displaySlotsMax = std::max(0, std::min(c->tune.displaySlots, PT_MAX_INFLIGHT - c->inflightMax));
  for(int i = 0; i < c->inflightMax + c->displaySlotsMax; ++i)
    if(hipStreamCreateWithFlags(&c->slots[i].stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->slots[i].accumDone, hipEventDisableTiming) != hipSuccess ||
       hipEventCreateWithFlags(&c->slots[i].countsDone, hipEventDisableTiming) != hipSuccess ||
       hipHostMalloc((void**)&c->slots[i].hCounts, sizeof(uint32_t) * CNT_STRIDE * (PT_MAX_DEPTH + 2)) != hipSuccess)
      return create_fail(PT_ERR_HIP, "hipStreamCreate / hipEventCreate failed", c);
  // defaults: sun & sky off, empty camera
  std::memset(&c->scene, 0, sizeof(c->scene));
  if(dev_alloc(c, c->dCounters, sizeof(Counters)) != PT_OK || hipMemset(c->dCounters.p, 0, sizeof(Counters)) != hipSuccess)
    return create_fail(PT_ERR_HIP, std::string(c->err), c);
  *out_ctx = c;
  return PT_OK;
}

int pt_destroy(pt_context* c)
{
  CTX_CHECK(c);
  (void)hipSetDevice(c->device);
  (void)sync_all(c);
  DevBuf* all[] = {&c->dMatLines, &c->dVertices, &c->dIndices, &c->dInstances, &c->dMaterials, &c->dLights, &c->dTexRecs, &c->dTexels, &c->dBvh, &c->dWide, &c->dTris, &c->dAlphaRecs, &c->dCNodes, &c->dRefit, &c->dCTlas, &c->dInstBlock, &c->dShadeTris, &c->dAlphaMats, &c->dAlphaMaps, &c->dPick, &c->dQueryRays, &c->dQueryHits, &c->dPathsChunk, &c->dPointsChunk, &c->dEnv,
                   &c->dTlas, &c->dTlasLeaves, &c->dInstTriBase, &c->dActive, &c->dInstNodeBase, &c->dInstPad, &c->dEnvAccel, &c->dFrame, &c->dSlotTile, &c->dCounters, &c->dRowMajor, &c->dRgba8,
                   &c->dMean, &c->dMips, &c->dGather, &c->dFullTiles, &c->dFullSlotTile, &c->dTileLocalIndex};
  for(DevBuf* b : all)
    dev_free(*b);
  stages_release(c);
  for(auto& fs : c->slots)
  {
    fs.release_paths();
    dev_free(fs.dCounts);
    dev_free(fs.dCountsDone);
    if(fs.accumDone)
      (void)hipEventDestroy(fs.accumDone);
    if(fs.countsDone)
      (void)hipEventDestroy(fs.countsDone);
    if(fs.hCounts)
      (void)hipHostFree(fs.hCounts);
    if(fs.stream)
      (void)hipStreamDestroy(fs.stream);
  }
  for(size_t i = 0; i < c->timers.cap; ++i)
  {
    (void)hipEventDestroy(c->timers.pend[i].a);
    (void)hipEventDestroy(c->timers.pend[i].b);
  }
  free(c->timers.pend);
  for(auto& ds : c->display)
  {
    if(ds.host)
      (void)hipHostFree(ds.host);
    if(ds.overflow)
      (void)hipHostFree(ds.overflow);
    if(ds.done)
      (void)hipEventDestroy(ds.done);
    if(ds.read)
      (void)hipEventDestroy(ds.read);
  }
  (void)hipStreamDestroy(c->stream);
  delete c;
  return PT_OK;
}

int pt_set_scene(pt_context* c, const pt_SceneDesc* d)
{
  CTX_CHECK(c);
  SceneRecords R;
  {
    std::string msg;
    const int   vrc = build_scene_records(d, R, msg, c->tune.texTile, c->tune.texGroups);
    if(vrc != PT_OK)
      return c->fail(vrc, "%s", msg.c_str());
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));
  c->hPrimBound = R.primBound;

  // ---- uploads
  int rc;
  if((rc = upload(c, c->dVertices, d->vertices, sizeof(pt_VertexAttributes) * size_t(d->numVertices))) != PT_OK) return rc;
  if((rc = upload(c, c->dIndices, d->indices, 4 * size_t(d->numIndices))) != PT_OK) return rc;
  c->hInstances = R.inst;
  if((rc = upload_instances(c)) != PT_OK) return rc;
  if((rc = upload(c, c->dMaterials, d->materials, sizeof(pt_GltfShadeMaterial) * size_t(d->numMaterials))) != PT_OK) return rc;
  {
    pt_Light dummy{};  // "cannot be null" (src/scene.cpp:329-330); never read because nbLights == 0 then
    if((rc = upload(c, c->dLights, d->numLights ? d->lights : &dummy, sizeof(pt_Light) * size_t(d->numLights ? d->numLights : 1))) != PT_OK) return rc;
    c->numLights = d->numLights;
  }
  if((rc = dev_alloc(c, c->dTexels, R.texels * 4)) != PT_OK)
  {  // the interleaved groups double the pool: without the memory for them the scene loads as with texGroups=0
    if(R.groups.empty())
      return rc;
    (void)hipGetLastError();
    std::string msg;
    R = SceneRecords();
    if((rc = build_scene_records(d, R, msg, c->tune.texTile, 0)) != PT_OK)
      return c->fail(rc, "%s", msg.c_str());
    if((rc = dev_alloc(c, c->dTexels, R.texels * 4)) != PT_OK)
      return rc;
  }
  if(d->numTextures == 0)
  {
    uint32_t white = 0xffffffffu;
    HIP_TRY(c, hipMemcpy(c->dTexels.p, &white, 4, hipMemcpyHostToDevice));
  }
  {
    std::vector<uint32_t> staged;  // one image at a time in its storage order
    for(uint32_t t = 0; t < d->numTextures; ++t)
    {
      const TexRec& tr = R.texRecs[t];
      const void*   src = d->textures[t].rgba8;
      if(tr.tiled)
      {
        staged.resize(size_t(tr.w) * tr.h);
        store_texture(staged.data(), tr, src);
        src = staged.data();
      }
      HIP_TRY(c, hipMemcpy((uint32_t*)c->dTexels.p + tr.offset, src, size_t(tr.w) * tr.h * 4, hipMemcpyHostToDevice));
    }
  }
  {
    std::vector<uint32_t> staged;  // one interleaved group at a time
    for(const SceneRecords::TexGroup& g : R.groups)
    {
      const TexRec& sh = R.texRecs[size_t(g.tex[0])];
      staged.assign(size_t(sh.w) * sh.h * size_t(g.layers), 0u);
      store_group(staged.data(), g, R.texRecs, d);
      HIP_TRY(c, hipMemcpy((uint32_t*)c->dTexels.p + g.offset, staged.data(), staged.size() * 4, hipMemcpyHostToDevice));
    }
  }
  if((rc = upload(c, c->dTexRecs, R.texRecs.data(), sizeof(TexRec) * R.texRecs.size())) != PT_OK) return rc;
  if((rc = upload(c, c->dMatLines, R.matLines.data(), sizeof(uint4) * R.matLines.size())) != PT_OK) return rc;
  if((rc = upload(c, c->dAlphaMaps, R.alphaMaps.data(), 4 * R.alphaMaps.size())) != PT_OK) return rc;
  if((rc = upload(c, c->dAlphaMats, R.alphaMats.data(), sizeof(AlphaMat) * R.alphaMats.size())) != PT_OK) return rc;
  c->numInstances = d->numNodes;
  c->numTris      = uint32_t(R.triTotal);
  c->qRatioDepths = 0;  // queue-size feedback of the previous scene
  // what pt_update_vertices needs -- the vertex count, every prim-mesh's vertex range, the positions -- replaced only now that the uploads succeeded: it
  // range-checks a device write against them
  c->numVertices = d->numVertices;
  c->hPrimMeshVerts.resize(2 * size_t(d->numPrimMeshes));
  for(uint32_t p = 0; p < d->numPrimMeshes; ++p)
  {
    c->hPrimMeshVerts[2 * p]     = d->primMeshes[p].vertexOffset;
    c->hPrimMeshVerts[2 * p + 1] = d->primMeshes[p].vertexCount;
  }
  c->hPositions.resize(3 * size_t(d->numVertices));
  for(uint32_t v = 0; v < d->numVertices; ++v)
    std::memcpy(&c->hPositions[3 * size_t(v)], d->vertices[v].position, 12);
  c->primTouched.assign(d->numPrimMeshes, 0);
  c->accelStale     = false;
  c->haveRefitTable = false;
  c->haveScene    = true;
  c->haveAccel    = false;
  refresh_scene_ptrs(c);
  return PT_OK;
}

int pt_set_camera(pt_context* c, const pt_SceneCamera* cam)
{
  CTX_CHECK(c);
  if(!cam)
    return c->fail(PT_ERR_INVALID, "pt_set_camera: null");
  int rc = flush_pending(c);  // frames already handed over keep the camera they were given
  if(rc != PT_OK)
    return rc;
  c->scene.camera = *cam;
  c->haveCamera   = true;
  return PT_OK;
}

int pt_set_sunsky(pt_context* c, const pt_SunAndSky* ss)
{
  CTX_CHECK(c);
  if(!ss)
    return c->fail(PT_ERR_INVALID, "pt_set_sunsky: null");
  int rc = flush_pending(c);
  if(rc != PT_OK)
    return rc;
  c->scene.sunsky = *ss;
  return PT_OK;
}

int pt_set_env(pt_context* c, const float* rgba, int w, int h, float* out_integral, float* out_average)
{
  CTX_CHECK(c);
  if(!rgba || w <= 0 || h <= 0)
    return c->fail(PT_ERR_INVALID, "pt_set_env: bad image");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));
  std::vector<pt_EnvAccel> accel(size_t(w) * h);
  float                    integral = 1.f, average = 1.f;
  if(pt_build_env_accel(rgba, w, h, accel.data(), &integral, &average) != PT_OK)
    return c->fail(PT_ERR_INVALID, "pt_build_env_accel failed");
  int rc;
  if((rc = upload(c, c->dEnv, rgba, sizeof(float) * 4 * size_t(w) * h)) != PT_OK) return rc;
  if((rc = upload(c, c->dEnvAccel, accel.data(), sizeof(pt_EnvAccel) * accel.size())) != PT_OK) return rc;
  c->scene.envW = w;
  c->scene.envH = h;
  c->haveEnv    = true;
  refresh_scene_ptrs(c);
  if(out_integral) *out_integral = integral;
  if(out_average) *out_average = average;
  return PT_OK;
}

int pt_set_variant(pt_context* c, int variant)
{
  CTX_CHECK(c);
  if(variant != PT_VARIANT_RAYQUERY && variant != PT_VARIANT_RTX)
    return c->fail(PT_ERR_INVALID, "pt_set_variant: %d", variant);
  int rc = flush_pending(c);  // frames already handed over keep the variant they were given
  if(rc != PT_OK)
    return rc;
  c->variant = variant;
  return PT_OK;
}

int pt_set_shard(pt_context* c, int rank, int nranks)
{
  CTX_CHECK(c);
  if(nranks < 1 || rank < 0 || rank >= nranks)
    return c->fail(PT_ERR_INVALID, "pt_set_shard: rank %d of %d", rank, nranks);
  c->rank   = rank;
  c->nranks = nranks;
  c->width = c->height = 0;  // force a re-layout on the next pt_resize
  return PT_OK;
}

// ---- launching frames ---------------------------------------------------------------------------------------
// the launch parameters that follow from the context; the caller adds the render state (st) and the frames of the launch (batch)
static FrameParams frame_params(const pt_context* c)
{
  FrameParams fp{};
  fp.width = c->width; fp.height = c->height; fp.tilesX = c->tilesX; fp.tilesY = c->tilesY; fp.rank = c->rank; fp.nranks = c->nranks;
  fp.numLocalTiles = c->numLocalTiles; fp.numSlots = c->numSlots; fp.variant = c->variant; fp.sample = 0;
  return fp;
}
// how many of the slots [firstK, lastK) (slot_at order) have no launch sequence running; a finished slot's `launched` is reset
static int idle_slots(pt_context* c, int firstK, int lastK)
{
  int idle = 0;
  for(int k = firstK; k < lastK; ++k)
  {
    FrameSlot& fs = slot_at(c, k);
    fs.launched   = fs.launched && hipEventQuery(fs.accumDone) == hipErrorNotReady;  // still running: its accumulate has not completed
    idle += fs.launched ? 0 : 1;
  }
  (void)hipGetLastError();  // hipErrorNotReady is not an error
  return idle;
}
// queue-size feedback: the counter block that came back from a launch of `paths` paths -> alive fraction at each of its `depths` bounces
static void take_queue_feedback(pt_context* c, const FrameSlot& fs, int depths, double paths)
{
  for(int d = 0; d < depths; ++d)
    c->qRatio[d] = double(fs.hCounts[size_t(d) * CNT_STRIDE + CNT_IN]) / paths;
  c->qRatioDepths = depths;
}
// The counter block of a frame slot is zero when a pass starts because the PREVIOUS pass's k_accumulate left it so (no fill kernel per sequence).  After a
// HIP error a sequence may have stopped short of that: stale queue sizes would make the next pass append past its queues.  Clear every slot's block --
// once nothing is running any more: if the wait fails the blocks are left alone and stay marked.
static int repair_counts(pt_context* c)
{
  const hipError_t e = sync_streams(c);
  (void)hipGetLastError();
  HIP_TRY(c, e);
  for(FrameSlot& fs : c->slots)
    if(fs.dCounts.p)
      HIP_TRY(c, fs.clear_counts());
  c->countsDirty = false;
  return PT_OK;
}

// Renderer::create is where the reference builds its pipelines (src/rayquery.cpp:63-92): everything a first frame would otherwise pay for happens
// here, untimed by definition.  Every frame slot's path state and queues are written once (first use of ~45 GB of fresh allocations), and one
// throw-away launch sequence runs on every slot's stream -- code objects of all stage kernels loaded, clocks up, scene / structure / textures
// pulled through the caches once, and the queue-size feedback (where k_tail takes over) seeded with the alive fractions of THIS scene
// instead of the 0.3-per-bounce guess.  Once per acceleration structure (pt_build_accel re-arms it).  Nothing the caller can observe changes: the accumulation image is cleared afterwards (pt_resize
// clears it anyway), the device counters are put back, statistics and frame numbering are untouched.  PT_TUNE warm=0 skips it.
static int warm_slots(pt_context* c)
{
  if(!c->tune.warm || !c->warmPending || !c->haveScene || !c->haveAccel || !c->haveCamera || !(c->haveEnv || c->scene.sunsky.in_use == 1) || c->numSlots == 0)
    return PT_OK;
  int rc;
  if(c->countsDirty && (rc = repair_counts(c)) != PT_OK)
    return rc;
  c->warmPending = false;  // once per scene: the de-scaling resizes of an interactive session (sample_example.cpp:410-413) must not stall on it
  if(c->scene.camera.nbLights < 0 || uint32_t(c->scene.camera.nbLights) > c->numLights)
    return PT_OK;  // pt_render_frame reports it
  Counters saved;
  HIP_TRY(c, hipMemcpy(&saved, c->dCounters.p, sizeof(Counters), hipMemcpyDeviceToHost));
  FrameParams fp = frame_params(c);
  fp.st.frame = 0; fp.st.maxDepth = 10; fp.st.maxSamples = 1; fp.st.fireflyClampThreshold = 1.0f; fp.st.hdrMultiplier = 1.0f;  // sample_example.hpp:162-174
  fp.st.debugging_mode = PT_DEBUG_NONE; fp.st.pbrMode = 0; fp.st.size[0] = c->width; fp.st.size[1] = c->height;
  fp.batch = uint32_t(std::min(c->batchMax, 8));
  StageTimers off;  // disabled: the warm-up never shows in the stage timings
  const int tailFrom = tail_from_depth(double(fp.batch) * double(c->numSlots), fp.st.maxDepth, c->tune.tailBelow, c->qRatio, 0);
  for(int k = 0; k < slot_total(c); ++k)
  {
    FrameSlot& fs = slot_at(c, k);
    fs.each_path_buffer([&](DevBuf& b, size_t) { (void)hipMemsetAsync(b.p, 0, b.bytes, fs.stream); });
  }
  for(int k = 0; k < slot_total(c); ++k)
  {
    FrameParams fk = fp;
    int         tk = tailFrom;
    if(k >= c->inflight)
    {  // a display slot holds one frame
      fk.batch = 1;
      tk       = tail_from_depth(double(c->numSlots), fp.st.maxDepth, c->tune.tailBelow, c->qRatio, 0);
    }
    pt_launch_frame(slot_at(c, k).stream, c->tune, c->scene, slot_at(c, k).rb, fk, &off, nullptr, nullptr, tk);
  }
  FrameSlot& f0 = c->slots[0];
  const int  nd = std::min(std::min(tailFrom + 1, int(fp.st.maxDepth)), PT_MAX_DEPTH);
  if(f0.hCounts)
    (void)hipMemcpyAsync(f0.hCounts, f0.rb.countsDone, sizeof(uint32_t) * CNT_STRIDE * size_t(nd), hipMemcpyDeviceToHost, f0.stream);
  hipError_t werr = hipSuccess;
  for(int k = 0; k < slot_total(c); ++k)
  {
    const hipError_t e = hipStreamSynchronize(slot_at(c, k).stream);
    werr               = werr == hipSuccess ? e : werr;
  }
  // whatever happened: the device counters and the accumulation image go back to what the caller left (best effort), and a failed warm-up is retried
  // by the next pt_resize instead of being silently skipped for the life of the scene
  const hipError_t r1 = hipMemcpy(c->dCounters.p, &saved, sizeof(Counters), hipMemcpyHostToDevice);
  const hipError_t r2 = hipMemset(c->dFrame.p, 0, c->dFrame.bytes);
  if(werr != hipSuccess || r1 != hipSuccess || r2 != hipSuccess)
  {
    c->warmPending = true;
    HIP_TRY(c, werr != hipSuccess ? werr : (r1 != hipSuccess ? r1 : r2));
  }
  if(f0.hCounts && c->qRatioDepths == 0)
    take_queue_feedback(c, f0, nd, double(fp.batch) * double(c->numSlots));
  return PT_OK;
}

int pt_resize(pt_context* c, int width, int height)
{
  CTX_CHECK(c);
  if(width <= 0 || height <= 0)
    return c->fail(PT_ERR_INVALID, "pt_resize: %dx%d", width, height);
  if(width == c->width && height == c->height)
    return PT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));
  stages_release(c);  // the denoiser's buffers, the guide planes and the history were sized for the old image
  c->tilesX = (width + PT_TILE - 1) / PT_TILE;
  c->tilesY = (height + PT_TILE - 1) / PT_TILE;
  std::vector<uint32_t> local;
  std::vector<uint32_t> perRank(c->nranks, 0);
  uint64_t              localPixels = 0;
  for(int ty = 0; ty < c->tilesY; ++ty)
    for(int tx = 0; tx < c->tilesX; ++tx)
    {
      int r = (tx + ty) % c->nranks;
      perRank[r]++;
      if(r == c->rank)
      {
        local.push_back(uint32_t(ty * c->tilesX + tx));
        localPixels += uint64_t(std::min(PT_TILE, width - tx * PT_TILE)) * uint64_t(std::min(PT_TILE, height - ty * PT_TILE));
      }
    }
  c->localPixels = localPixels;
  c->numLocalTiles   = uint32_t(local.size());
  c->maxTilesPerRank = 0;
  for(uint32_t v : perRank)
    c->maxTilesPerRank = v > c->maxTilesPerRank ? v : c->maxTilesPerRank;
  c->numSlots = c->numLocalTiles * 1024u;

  int rc;
  // frames per batch: the tuning value, bounded so that one frame slot's path state stays below 2^26 paths (~11 GB):
  // 32 frames of a full 1080p image, 64 of an 8-GPU shard (measured best for both, profiles/r01_scaling_estimate.txt)
  c->batchMax = std::max(1, std::min(c->tune.batch, int((1u << 26) / (c->numSlots ? c->numSlots : 1u))));
  // In-flight path state: 9 float4 arrays + 9 index queues per path slot, times the batch, times the frame slots -- 38 GB for a 1080p image at
  // the defaults, sized for 288 GB of HBM.  It is a budget, not a requirement: PT_TUNE stateGB=<n> (or what hipMemGetInfo reports as free,
  // minus a reserve) caps it, and an allocation that still fails halves the batch / drops frame slots and retries, down to one frame on
  // one slot, before PT_ERR_OOM is reported.  Smaller batches only cost throughput, never results.
  const size_t perPath = FrameSlot::bytesPerPath;
  c->inflight          = c->inflightMax;
  c->displaySlots      = c->displaySlotsMax;
  // (Round 6 tried a policy by shard size here -- two frame slots for a shard of at most 300 k pixels, what PT_TUNE inflight=2 showed on a 1/8 shard of a
  // 1080p image at 20 steps: +5 % there, but -9 % at the configuration's own 256 steps, where four full batches want four slots: 89 % -> 81 % predicted
  // efficiency at 8 GPUs (profiles/r06_shard_policy_experiment.txt).  Not adopted: the slot count stays what the context was created with.)
  {
    // what is free now PLUS what the frame slots already hold (those buffers are re-used or released below): a repeated pt_resize at the same
    // size must arrive at the same batch, not at half of it.  A failed query means "no cap" -- the retry loop below still shrinks on a failed allocation.
    size_t freeB = 0, totalB = 0, held = 0;
    const bool haveInfo = hipMemGetInfo(&freeB, &totalB) == hipSuccess;
    (void)hipGetLastError();
    for(FrameSlot& fs : c->slots)
      held += fs.bytes_held();
    const double budget = c->tune.stateMB > 0 ? c->tune.stateMB * 1e6 : c->tune.stateGB > 0 ? c->tune.stateGB * 1e9 : (haveInfo ? (double(freeB) + double(held)) * 0.85 : 1e30);
    auto need = [&]() { return double(perPath) * double(c->numSlots ? c->numSlots : 1) * (double(c->batchMax) * c->inflight + c->displaySlots); };
    if(need() > budget)
      c->displaySlots = 0;  // the one-frame display slots go first
    while(c->batchMax > 1 && need() > budget)
      c->batchMax = (c->batchMax + 1) / 2;
    while(c->inflight > 1 && need() > budget)
      c->inflight = (c->inflight + 1) / 2;
    if((c->tune.stateMB > 0 || c->tune.stateGB > 0) && need() > budget)  // an explicit cap that one frame on one slot exceeds (a cap derived
      return c->fail(PT_ERR_OOM, "pt_resize: the path state of one %dx%d frame (%.0f bytes) exceeds the configured budget (%.0f bytes)", width, height, need(), budget);  // from the free memory is left to the allocations below)
  }
  for(;;)
  {
    bool         ok = true;
    for(int k = 0; k < slot_total(c) && ok; ++k)
    {
      FrameSlot& fs = slot_at(c, k);
      ok            = fs.alloc(size_t(c->numSlots ? c->numSlots : 1) * size_t(k < c->inflight ? c->batchMax : 1));
      if(ok)
        HIP_TRY(c, fs.clear_counts());
    }
    if(ok)
    {  // slots that dropped out (a smaller budget than at the last pt_resize) give their buffers back
      for(int i = 0; i < PT_MAX_INFLIGHT; ++i)
      {
        const bool used = i < c->inflight || (i >= c->inflightMax && i < c->inflightMax + c->displaySlots);
        if(!used)
          c->slots[i].release_paths();
      }
      break;
    }
    (void)hipGetLastError();
    for(FrameSlot& fs : c->slots)
      fs.release_paths();  // everything, before retrying smaller
    if(c->displaySlots > 0)
      c->displaySlots = 0;
    else if(c->batchMax > 1)
      c->batchMax = (c->batchMax + 1) / 2;
    else if(c->inflight > 1)
      c->inflight = (c->inflight + 1) / 2;
    else
      return c->fail(PT_ERR_OOM, "pt_resize: not enough device memory for the path state of one %dx%d frame (%zu bytes per path)", width, height, perPath);
  }
  if((rc = dev_alloc(c, c->dFrame, sizeof(float4) * size_t(c->maxTilesPerRank ? c->maxTilesPerRank : 1) * 1024u)) != PT_OK) return rc;
  if((rc = upload(c, c->dSlotTile, local.data(), 4 * local.size())) != PT_OK) return rc;
  HIP_TRY(c, hipMemset(c->dFrame.p, 0, c->dFrame.bytes));
  if((rc = dev_alloc(c, c->dRowMajor, sizeof(float4) * size_t(width) * height)) != PT_OK) return rc;
  HIP_TRY(c, hipMemset(c->dRowMajor.p, 0, sizeof(float4) * size_t(width) * height));
  if((rc = dev_alloc(c, c->dRgba8, 4 * size_t(width) * height)) != PT_OK) return rc;
  if((rc = dev_alloc(c, c->dMean, 3 * sizeof(double))) != PT_OK) return rc;

  c->width    = width;
  c->height   = height;
  c->haveFull = false;
  for(int k = 0; k < slot_total(c); ++k)
    slot_at(c, k).bind((float4*)c->dFrame.p, (uint32_t*)c->dSlotTile.p, (Counters*)c->dCounters.p);
  return warm_slots(c);
}

int pt_render_frame(pt_context* c, const pt_RtxState* st)
{
  CTX_CHECK(c);
  if(!st)
    return c->fail(PT_ERR_INVALID, "pt_render_frame: null state");
  if(!c->haveScene || !c->haveAccel)
    return c->fail(PT_ERR_STATE, "pt_render_frame %s", c->no_accel());
  if(!c->haveEnv && c->scene.sunsky.in_use != 1)
    return c->fail(PT_ERR_STATE, "pt_render_frame without an environment (pt_set_env) or sun & sky");
  if(c->width == 0)
    return c->fail(PT_ERR_STATE, "pt_render_frame before pt_resize");
  if(st->size[0] != c->width || st->size[1] != c->height)
    return c->fail(PT_ERR_INVALID, "RtxState.size %dx%d != pt_resize %dx%d", st->size[0], st->size[1], c->width, c->height);
  if(st->maxSamples < 1 || st->maxDepth < 0 || st->maxDepth > PT_MAX_DEPTH || st->frame < 0)
    return c->fail(PT_ERR_INVALID, "RtxState: maxSamples %d maxDepth %d (limit %d) frame %d", st->maxSamples, st->maxDepth, PT_MAX_DEPTH, st->frame);
  // the lights buffer holds numLights records (pt_set_scene); the shader indexes it with camera.nbLights (pathtrace.glsl:120-121), and the two
  // arrive through independent calls
  if(c->scene.camera.nbLights < 0 || uint32_t(c->scene.camera.nbLights) > c->numLights)
    return c->fail(PT_ERR_INVALID, "camera.nbLights = %d but the scene holds %u lights", c->scene.camera.nbLights, c->numLights);
  HIP_TRY(c, hipSetDevice(c->device));
  if(c->numSlots == 0)
    return PT_OK;
  pt_RtxState a = *st, b = c->pendState;
  a.frame = b.frame = 0;
  const bool joins = c->pendCount > 0 && c->pendCount < c->batchMax && std::memcmp(&a, &b, sizeof(a)) == 0 && st->frame == c->pendState.frame + c->pendCount;
  int rc;
  if(!joins && (rc = flush_pending(c)) != PT_OK)
    return rc;
  if(c->pendCount == 0)
    c->pendState = *st;
  c->pendCount++;
  c->haveFull = false;
  c->stats.samples += uint64_t(st->maxSamples) * c->localPixels;
  if(c->pendCount >= c->batchMax)
    return flush_pending(c);
  return PT_OK;
}

}  // extern "C"

// one launch sequence of flush_pending: a run of the pending frames on a frame slot, or a band of one frame's tiles
struct Piece {
  FrameSlot*    fs;
  RenderBuffers rb;  // the slot's, or its view of a band
  FrameParams   fp;
  int           tailFrom;  // where k_tail takes over (tail_from_depth)
  uint32_t      paths;
};
// Launches the frames handed to pt_render_frame that have not been launched yet, as one or several launch sequences on the next frame slots' streams.
int flush_pending(pt_context* c)
{
  if(c->pendCount == 0)
    return PT_OK;
  int rc;
  if(c->countsDirty && (rc = repair_counts(c)) != PT_OK)
    return rc;
  FrameParams fp = frame_params(c);
  fp.st          = c->pendState;
  // A batch is cut into as many pieces as there are idle frame slots (separate streams), so that a short run of frames -- or the first
  // batch of a long one -- has several launch sequences overlapping instead of one chain of dependent kernels.  In the steady state of a
  // long run every slot is busy and a full batch goes out as one sequence.
  int       parts = 1;
  const int total = c->pendCount;
  if(total >= 4)
  {
    const int freeSlots = idle_slots(c, 0, c->inflight);
    // a partial flush (the caller is waiting) is cut fine; a full batch only when the GPU is idle (the first batch of a run) -- later ones
    // find busy slots and go out whole, so the steady state of a long run works on full batches
    const int minPart = total < c->batchMax ? 2 : total;  // a full batch is never split (2-7 % slower at 96-256 frames, profiles/README.md)
    parts = std::max(1, std::min(freeSlots, total / minPart));
  }
  // A launch of ONE frame while nothing else runs (a display loop that waits for every image) is cut the other way: into bands of the frame's
  // tiles, one launch sequence per idle slot.  A band addresses its part of the tile list, of the accumulation image and of nothing else, so it
  // is an ordinary launch with shifted base pointers; the bands' late, thin bounces overlap each other's full ones (profiles/r04z_*).
  int bands = 1;
  if(total == 1 && c->tune.bands > 1 && !c->timers.enabled)
  {
    const int idle = idle_slots(c, 0, slot_total(c));
    if(idle == slot_total(c))  // with frames in flight the slots are the pipeline: one sequence per frame
      bands = std::max(1, std::min(std::min(idle, c->tune.bands), int(c->numLocalTiles / uint32_t(c->tune.bandTiles))));
  }
  c->pendCount          = 0;
  c->renderedSinceCheck = true;
  // queue-size feedback: take the counters of the newest launch sequence that has finished
  for(FrameSlot& fs : c->slots)
    if(fs.countsDone && fs.countsSeq > c->qRatioSeq && fs.countsPaths > 0 && hipEventQuery(fs.countsDone) == hipSuccess)
    {
      take_queue_feedback(c, fs, std::min(fs.countsDepths, PT_MAX_DEPTH), double(fs.countsPaths));
      c->qRatioSeq = fs.countsSeq;
    }
  (void)hipGetLastError();  // hipErrorNotReady is not an error
  // where k_tail takes over in a piece: the first bounce whose queue is expected to hold <= tailBelow paths.  Expectation = the piece's paths x the
  // alive fraction observed at that bounce; bounces beyond the observed ones continue the last observed shrink factor; before anything was
  // observed a shrink of 0.3 per bounce is assumed.  A wrong guess costs time, never results.
  auto tail_from = [&](uint32_t paths) { return tail_from_depth(double(paths), fp.st.maxDepth, c->tune.tailBelow, c->qRatio, c->qRatioDepths); };
  std::vector<Piece> pieces;
  for(int b = 0; b < bands && bands > 1; ++b)
  {
    const uint32_t t0 = uint32_t(uint64_t(c->numLocalTiles) * uint64_t(b) / uint64_t(bands)), t1 = uint32_t(uint64_t(c->numLocalTiles) * uint64_t(b + 1) / uint64_t(bands));
    Piece pc{&slot_at(c, int(c->displayCounter++ % uint64_t(slot_total(c)))), {}, fp, 0, (t1 - t0) * 1024u};
    pc.fp.batch         = 1;
    pc.fp.numLocalTiles = t1 - t0;
    pc.fp.numSlots      = pc.paths;
    pc.rb               = pc.fs->rb;
    pc.rb.slotTile += t0;
    pc.rb.frame += size_t(t0) * 1024u;
    pc.tailFrom = tail_from(pc.paths);
    pieces.push_back(pc);
  }
  for(int p = 0, done = 0; p < parts && bands == 1; ++p)
  {
    // (equal pieces: sizes falling 4 : 3 : 2 : 1, meant to let the streams drift apart so that trace and shade stages overlap, measured 5 % slower,
    // eight pieces on eight slots 20 % slower, profiles/r04d_*)
    const int n = (total - done) / (parts - p);
    // a launch of ONE frame (the display loop flushes per frame) rotates over the batch slots and the display slots, a batch over the batch slots
    FrameSlot& fs = (total == 1 && c->displaySlots > 0) ? slot_at(c, int(c->displayCounter++ % uint64_t(slot_total(c)))) : c->slots[c->frameCounter++ % uint64_t(c->inflight)];
    Piece      pc{&fs, fs.rb, fp, 0, uint32_t(n) * c->numSlots};
    pc.fp.st.frame = c->pendState.frame + done;
    pc.fp.batch    = uint32_t(n);
    pc.tailFrom    = tail_from(pc.paths);
    pieces.push_back(pc);
    done += n;
  }
  // interleaved submission needs every piece to have exactly one accumulate step, and the stage timers record their events in launch order
  const bool                       interleave = pieces.size() > 1 && fp.st.maxSamples == 1 && !c->timers.enabled;
  std::vector<std::vector<PtStep>> plans(pieces.size());
  for(size_t q = 0; q < pieces.size(); ++q)
  {
    const Piece& pc = pieces[q];
    pt_plan_frame(plans[q], pc.fs->stream, c->tune, c->scene, pc.rb, pc.fp, &c->timers, c->lastAccum, pc.fs->accumDone, pc.tailFrom);
    c->lastAccum     = pc.fs->accumDone;
    pc.fs->launched  = true;
    if(!interleave)
    {  // one sequence after the other
      for(PtStep& st : plans[q])
        st.fn();
      plans[q].clear();
    }
  }
  if(interleave)
  {  // stage by stage in turn over the pieces: every stream gets its first kernels at once, the host stays ahead of all of them; a piece's
     // accumulate step (it waits on the previous piece's event) is never issued before the previous piece's
    std::vector<size_t> at(plans.size(), 0);
    std::vector<char>   accumIssued(plans.size(), 0);
    for(bool more = true; more;)
    {
      more = false;
      for(size_t q = 0; q < plans.size(); ++q)
      {
        if(at[q] >= plans[q].size())
          continue;
        PtStep& st = plans[q][at[q]];
        if(st.accum && q > 0 && !accumIssued[q - 1])
        {
          more = true;
          continue;
        }
        st.fn();
        if(st.accum)
          accumIssued[q] = 1;
        ++at[q];
        more = more || at[q] < plans[q].size();
      }
    }
  }
  for(const Piece& pc : pieces)
  {
    FrameSlot& fs = *pc.fs;
    if(fs.hCounts && fp.st.debugging_mode != PT_DEBUG_HEATMAP)
    {
      fs.countsDepths = std::min(std::min(pc.tailFrom + 1, int(fp.st.maxDepth)), PT_MAX_DEPTH);  // the bounce k_tail starts at still has its input count
      fs.countsPaths  = pc.paths;
      if(hipMemcpyAsync(fs.hCounts, fs.rb.countsDone, sizeof(uint32_t) * CNT_STRIDE * size_t(fs.countsDepths), hipMemcpyDeviceToHost, fs.stream) == hipSuccess &&
         hipEventRecord(fs.countsDone, fs.stream) == hipSuccess)
        fs.countsSeq = ++c->launchSeq;
      else
        fs.countsSeq = 0;
    }
  }
  HIP_TRY(c, hipGetLastError());
  return PT_OK;
}
extern "C" {

int pt_synchronize(pt_context* c)
{
  CTX_CHECK(c);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));
  return check_traversal(c);
}

}  // extern "C"
// The row-major accumulation image (dRowMajor), enqueued on the context's stream behind the frames rendered so far: what pt_read_accum copies out and
// what the display pass and the denoiser (pt_denoise.hip) read
int untile_to_rowmajor(pt_context* c)
{
  int rc = flush_pending(c);
  if(rc != PT_OK)
    return rc;
  // frames run on their own streams; the last accumulate (itself ordered after all earlier ones) gates the readback
  if(c->lastAccum)
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->lastAccum, 0));
  if(c->haveFull)
    pt_launch_untile(c->stream, (const float4*)c->dFullTiles.p, (const uint32_t*)c->dFullSlotTile.p, uint32_t(c->tilesX) * c->tilesY, c->tilesX, c->width, c->height,
                     (float4*)c->dRowMajor.p);
  else
    pt_launch_untile(c->stream, (const float4*)c->dFrame.p, (const uint32_t*)c->dSlotTile.p, c->numLocalTiles, c->tilesX, c->width, c->height, (float4*)c->dRowMajor.p);
  HIP_TRY(c, hipGetLastError());
  return PT_OK;
}
extern "C" {

int pt_read_accum(pt_context* c, float* out)
{
  CTX_CHECK(c);
  if(!out)
    return c->fail(PT_ERR_INVALID, "pt_read_accum: null");
  if(c->width == 0)
    return c->fail(PT_ERR_STATE, "pt_read_accum before pt_resize");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = untile_to_rowmajor(c);
  if(rc != PT_OK)
    return rc;
  HIP_TRY(c, hipMemcpyAsync(out, c->dRowMajor.p, sizeof(float4) * size_t(c->width) * c->height, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, sync_all(c));
  return check_traversal(c);
}

int pt_write_accum(pt_context* c, const float* in)
{
  CTX_CHECK(c);
  if(!in)
    return c->fail(PT_ERR_INVALID, "pt_write_accum: null");
  if(c->width == 0)
    return c->fail(PT_ERR_STATE, "pt_write_accum before pt_resize");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));  // launches what is pending and waits: the restored image replaces everything rendered so far
  HIP_TRY(c, hipMemcpyAsync(c->dRowMajor.p, in, sizeof(float4) * size_t(c->width) * c->height, hipMemcpyHostToDevice, c->stream));
  pt_launch_retile(c->stream, (const float4*)c->dRowMajor.p, (const uint32_t*)c->dSlotTile.p, c->numLocalTiles, c->tilesX, c->width, c->height, (float4*)c->dFrame.p);
  HIP_TRY(c, hipGetLastError());
  // the staging image keeps only what the untile writes back: pixels of other ranks read back as zero, as after rendering
  HIP_TRY(c, hipMemsetAsync(c->dRowMajor.p, 0, sizeof(float4) * size_t(c->width) * c->height, c->stream));
  HIP_TRY(c, sync_all(c));
  c->haveFull = false;
  return PT_OK;
}

int pt_pick(pt_context* c, float pick_x, float pick_y, const float* view_inverse, const float* proj_inverse, pt_PickResult* out)
{
  CTX_CHECK(c);
  if(!view_inverse || !proj_inverse || !out)
    return c->fail(PT_ERR_INVALID, "pt_pick: null");
  if(!c->haveScene || !c->haveAccel)
    return c->fail(PT_ERR_STATE, "pt_pick %s", c->no_accel());
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;
  if((rc = dev_alloc(c, c->dPick, sizeof(pt_PickResult))) != PT_OK)
    return rc;
  pt_launch_pick(c->stream, c->scene, pick_x, pick_y, view_inverse, proj_inverse, (pt_PickResult*)c->dPick.p, (Counters*)c->dCounters.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, c->dPick.p, sizeof(pt_PickResult), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, sync_all(c));
  c->renderedSinceCheck = true;  // the pick's own walk counts into the same counter
  return check_traversal(c);
}

}  // extern "C"
// The offscreen image as post.frag samples it, enqueued on the context's stream from the row-major accumulation image (untile_to_rowmajor): level 0 is
// the accumulation image itself, or a viewport-sized image with it in the top-left corner (texels outside: zero); levels 1.. only with `chain`
// (src/sample_example.cpp:423-427 generates the chain only with auto-exposure): extent max(1, e / 2), floor(log2(max(w, h))) + 1 levels.
// readDone (may be null): recorded once the accumulation image has been read, and made the event the next frame's accumulate step waits for.
// display_chain chooses level 0 -- the accumulation image; display_levels is everything after that choice, shared with the denoised pass
// (pt_denoise.hip), whose level 0 is the filtered image.
int display_chain(pt_context* c, int dispW, int dispH, bool chain, hipEvent_t readDone, MipView& mv)
{
  if(c->width == 0)
    return c->fail(PT_ERR_STATE, "pt_tonemap before pt_resize");
  if(dispW < c->width || dispH < c->height || dispW > 32768 || dispH > 32768)
    return c->fail(PT_ERR_INVALID, "pt_tonemap_zoom: the viewport must be at least as large as the accumulation image");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = untile_to_rowmajor(c);
  if(rc != PT_OK)
    return rc;
  if(readDone)
  {
    HIP_TRY(c, hipEventRecord(readDone, c->stream));
    c->lastAccum = readDone;
  }
  return display_levels(c, (const float4*)c->dRowMajor.p, dispW, dispH, chain, mv);
}
int display_levels(pt_context* c, const float4* image, int dispW, int dispH, bool chain, MipView& mv)
{
  int        rc;
  const bool padded = dispW != c->width || dispH != c->height;
  size_t     texels = padded ? size_t(dispW) * dispH : 0, offset = texels;
  int        lw = dispW, lh = dispH, levels = 1;
  if(chain)
    for(int m = dispW > dispH ? dispW : dispH; m > 1; m >>= 1)
    {
      lw = lw > 1 ? lw / 2 : 1;
      lh = lh > 1 ? lh / 2 : 1;
      texels += size_t(lw) * lh;
      levels++;
    }
  if(texels && (rc = dev_alloc(c, c->dMips, sizeof(float4) * texels)) != PT_OK)
    return rc;
  float4* pool = (float4*)c->dMips.p;
  if(padded)
    pt_launch_pad_corner(c->stream, image, c->width, c->height, pool, dispW, dispH);
  mv.level[0] = padded ? pool : image;
  mv.w[0] = dispW; mv.h[0] = dispH; mv.n = levels;
  for(int i = 1; i < levels; ++i)
  {
    mv.w[i]     = mv.w[i - 1] > 1 ? mv.w[i - 1] / 2 : 1;
    mv.h[i]     = mv.h[i - 1] > 1 ? mv.h[i - 1] / 2 : 1;
    mv.level[i] = pool + offset;
    pt_launch_blit_linear(c->stream, mv.level[i - 1], mv.w[i - 1], mv.h[i - 1], pool + offset, mv.w[i], mv.h[i]);
    offset += size_t(mv.w[i]) * mv.h[i];
  }
  HIP_TRY(c, hipGetLastError());
  return PT_OK;
}
// The level texture(inImage, uvCoords * zoom, bias) reads, bias 0..7 (post.frag:82-83, :101), by the Vulkan rules "Scale Factor Operation, LOD
// Operation and Image Level(s) Selection": in the full-screen pass uvCoords * zoom advances `zoom` texels of level 0 per pixel on both axes, so
// lambda_base = log2(zoom); lambda = clamp(lambda_base + bias, minLod = 0, maxLod = FLT_MAX) (the sampler of render_output.cpp:98-100); with
// mipmapMode NEAREST the level is the nearest integer to min(lambda, levels - 1).  Computed here so that the kernel needs no log2.
static void select_levels(MipView& mv, float zoom)
{
  const float base = log2f(zoom);
  for(int i = 0; i < 8; ++i)
  {
    const float lambda = fmaxf(base + float(i), 0.0f);  // fmaxf: 0 for a NaN (zoom < 0)
    mv.sel[i]          = int(fminf(floorf(lambda + 0.5f), float(mv.n - 1)));
  }
}
// The display pass enqueued on the context's stream, ending with the copy of the RGBA8 image to `out` (host memory; the caller synchronises).
// readDone: recorded once the accumulation image has been read, and made the event the next frame's accumulate step waits for -- frames
// rendered after this call may then overlap the rest of the pass.
static int enqueue_tonemap(pt_context* c, const pt_Tonemapper* tm, int dispW, int dispH, uint8_t* out, hipEvent_t readDone)
{
  if(!tm || !out)
    return c->fail(PT_ERR_INVALID, "pt_tonemap: null");
  int     rc;
  MipView mv{};
  if((rc = display_chain(c, dispW, dispH, (tm->autoExposure & 1) != 0, readDone, mv)) != PT_OK)
    return rc;
  return display_finish(c, tm, mv, dispW, dispH, out);
}
// ... from the offscreen image on: the tonemap kernel and the copy
int display_finish(pt_context* c, const pt_Tonemapper* tm, MipView& mv, int dispW, int dispH, uint8_t* out)
{
  int rc;
  select_levels(mv, tm->zoom);
  if((rc = dev_alloc(c, c->dRgba8, 4 * size_t(dispW) * dispH)) != PT_OK)
    return rc;
  pt_launch_tonemap(c->stream, mv, *tm, (uint32_t*)c->dRgba8.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, c->dRgba8.p, 4 * size_t(dispW) * dispH, hipMemcpyDeviceToHost, c->stream));
  return PT_OK;
}
extern "C" {
int pt_tonemap_zoom(pt_context* c, const pt_Tonemapper* tm, int dispW, int dispH, uint8_t* out)
{
  CTX_CHECK(c);
  int rc = enqueue_tonemap(c, tm, dispW, dispH, out, nullptr);
  if(rc != PT_OK)
    return rc;
  HIP_TRY(c, sync_all(c));
  return check_traversal(c);
}
int pt_tonemap(pt_context* c, const pt_Tonemapper* tm, uint8_t* out)
{
  CTX_CHECK(c);
  return pt_tonemap_zoom(c, tm, c->width, c->height, out);
}

int pt_tonemap_begin(pt_context* c, const pt_Tonemapper* tm, int dispW, int dispH)
{
  CTX_CHECK(c);
  if(c->displayTail - c->displayHead >= PT_DISPLAY_RING)
    return c->fail(PT_ERR_STATE, "pt_tonemap_begin: %d images are waiting for pt_tonemap_end", PT_DISPLAY_RING);
  if(dispW <= 0 || dispH <= 0 || dispW > 32768 || dispH > 32768)
    return c->fail(PT_ERR_INVALID, "pt_tonemap_begin: viewport %dx%d", dispW, dispH);
  if(c->overflowSeen)  // known already: nothing is enqueued (without a synchronisation pt_tonemap_end is the call that finds out)
    return report_overflow(c);
  HIP_TRY(c, hipSetDevice(c->device));
  pt_context::DisplaySlot& ds    = c->display[c->displayTail % PT_DISPLAY_RING];
  const size_t             bytes = 4 * size_t(dispW) * dispH;
  if(ds.bytes < bytes)
  {
    if(ds.host)
      (void)hipHostFree(ds.host);
    ds.host  = nullptr;
    ds.bytes = 0;
    HIP_TRY(c, hipHostMalloc((void**)&ds.host, bytes, hipHostMallocDefault));
    ds.bytes = bytes;
  }
  if(!ds.done)
    HIP_TRY(c, hipEventCreateWithFlags(&ds.done, hipEventDisableTiming));
  if(!ds.read)
    HIP_TRY(c, hipEventCreateWithFlags(&ds.read, hipEventDisableTiming));
  if(!ds.overflow)
    HIP_TRY(c, hipHostMalloc((void**)&ds.overflow, sizeof(unsigned), hipHostMallocDefault));
  int rc = enqueue_tonemap(c, tm, dispW, dispH, ds.host, ds.read);
  if(rc != PT_OK)
    return rc;
  // behind the frames the pass reads (untile_to_rowmajor waits for them): the overflow counter, without a synchronisation here
  HIP_TRY(c, hipMemcpyAsync(ds.overflow, (const char*)c->dCounters.p + offsetof(Counters, stackOverflow), sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipEventRecord(ds.done, c->stream));
  ds.used = bytes;
  c->displayTail++;
  return PT_OK;
}
int pt_tonemap_pending(pt_context* c)
{
  return c ? int(c->displayTail - c->displayHead) : 0;
}
int pt_tonemap_end(pt_context* c, uint8_t* out)
{
  CTX_CHECK(c);
  if(!out)
    return c->fail(PT_ERR_INVALID, "pt_tonemap_end: null");
  if(c->displayHead == c->displayTail)
    return c->fail(PT_ERR_STATE, "pt_tonemap_end without a pending pt_tonemap_begin");
  HIP_TRY(c, hipSetDevice(c->device));
  pt_context::DisplaySlot& ds = c->display[c->displayHead % PT_DISPLAY_RING];
  HIP_TRY(c, hipEventSynchronize(ds.done));
  std::memcpy(out, ds.host, ds.used);
  c->displayHead++;
  if(*ds.overflow > c->overflowSeen)
    c->overflowSeen = *ds.overflow;
  return c->overflowSeen ? report_overflow(c) : PT_OK;
}

int pt_local_shard(pt_context* c, void** device_ptr, size_t* bytes, int* num_local_tiles, int* max_tiles_per_rank)
{
  CTX_CHECK(c);
  if(c->width == 0)
    return c->fail(PT_ERR_STATE, "pt_local_shard before pt_resize");
  int rc = flush_pending(c);
  if(rc != PT_OK)
    return rc;
  if(c->renderedSinceCheck)  // the shard leaves the library here: the frames it holds must not have lost geometry
  {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
  }
  if((rc = check_traversal(c)) != PT_OK)
    return rc;
  if(device_ptr) *device_ptr = c->dFrame.p;
  if(bytes) *bytes = sizeof(float4) * size_t(c->maxTilesPerRank) * 1024u;
  if(num_local_tiles) *num_local_tiles = int(c->numLocalTiles);
  if(max_tiles_per_rank) *max_tiles_per_rank = int(c->maxTilesPerRank);
  return PT_OK;
}

int pt_scatter_shards(pt_context* c, const void* gathered_dev, int nranks)
{
  CTX_CHECK(c);
  if(!gathered_dev || nranks != c->nranks)
    return c->fail(PT_ERR_INVALID, "pt_scatter_shards: nranks %d != %d", nranks, c->nranks);
  if(c->width == 0)
    return c->fail(PT_ERR_STATE, "pt_scatter_shards before pt_resize");
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t        nt = uint32_t(c->tilesX) * c->tilesY;
  std::vector<uint32_t> localIndex(nt), identity(nt), next(nranks, 0);
  for(uint32_t gt = 0; gt < nt; ++gt)
  {
    int r          = (int(gt % c->tilesX) + int(gt / c->tilesX)) % nranks;
    localIndex[gt] = next[r]++;
    identity[gt]   = gt;
  }
  int rc;
  if((rc = dev_alloc(c, c->dFullTiles, sizeof(float4) * size_t(nt) * 1024u)) != PT_OK) return rc;
  if((rc = upload(c, c->dTileLocalIndex, localIndex.data(), 4 * size_t(nt))) != PT_OK) return rc;
  if((rc = upload(c, c->dFullSlotTile, identity.data(), 4 * size_t(nt))) != PT_OK) return rc;
  pt_launch_scatter_tiles(c->stream, (const float4*)gathered_dev, nranks, int(c->maxTilesPerRank), c->tilesX, c->tilesY, (const uint32_t*)c->dTileLocalIndex.p,
                          (float4*)c->dFullTiles.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, sync_all(c));
  c->haveFull = true;
  return PT_OK;
}

// internal hooks of pt_comm.cpp (hidden: not part of the ABI)
// traversal: check_traversal of the shard (PT_ERR_STATE after an overflow).  pt_gather_shards still takes part in the collective -- a rank
// that left it would stall its peers -- and returns this code afterwards.
__attribute__((visibility("hidden"))) int pt_comm_internal_shard(pt_context* c, void** shard, size_t* bytes, int* rank, int* nranks, int root, void** gatherBuf, hipStream_t* stream, int* device,
                                                                  int* traversal)
{
  CTX_CHECK(c);
  if(c->width == 0)
    return c->fail(PT_ERR_STATE, "pt_gather_shards before pt_resize");
  if(root < 0 || root >= c->nranks)
    return c->fail(PT_ERR_INVALID, "pt_gather_shards: root %d of %d ranks", root, c->nranks);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));  // the shard is complete; the gather is enqueued on the context's stream
  *traversal = check_traversal(c);
  *shard  = c->dFrame.p;
  *bytes  = sizeof(float4) * size_t(c->maxTilesPerRank) * 1024u;
  *rank   = c->rank;
  *nranks = c->nranks;
  *stream = c->stream;
  *device = c->device;
  *gatherBuf       = nullptr;
  c->gatherEnqueued = false;
  if(c->rank == root)
  {  // only the root holds the nranks x shard buffer (133 MB for a 4K image on 8 GPUs)
    int rc = dev_alloc(c, c->dGather, *bytes * size_t(c->nranks));
    if(rc != PT_OK)
      return rc;
    *gatherBuf        = c->dGather.p;
    c->gatherEnqueued = true;
  }
  return PT_OK;
}
__attribute__((visibility("hidden"))) void pt_comm_internal_fail(pt_context* c, int code, const char* msg)
{
  c->gatherEnqueued = false;
  c->fail(code, "%s", msg);
}

int pt_gather_finish(pt_context* c)
{
  CTX_CHECK(c);
  if(!c->gatherEnqueued || !c->dGather.p)
    return c->fail(PT_ERR_STATE, "pt_gather_finish without a pt_gather_shards that this context enqueued as the root");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->gatherEnqueued = false;
  return pt_scatter_shards(c, c->dGather.p, c->nranks);
}

int pt_set_profiling(pt_context* c, int enable)
{
  CTX_CHECK(c);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));
  pt_timers_collect(&c->timers);
  c->timers.enabled = enable != 0;
  return PT_OK;
}

int pt_get_stats(pt_context* c, pt_Stats* out)
{
  CTX_CHECK(c);
  if(!out)
    return c->fail(PT_ERR_INVALID, "pt_get_stats: null");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));
  pt_timers_collect(&c->timers);
  Counters k{};
  HIP_TRY(c, hipMemcpy(&k, c->dCounters.p, sizeof(k), hipMemcpyDeviceToHost));
  c->renderedSinceCheck = false;
  c->overflowSeen       = k.stackOverflow;
  if(k.stackOverflow)
    return report_overflow(c);
  pt_Stats s = c->stats;
  s.closestRays = k.closestRays; s.shadowRays = k.shadowRays; s.shadedHits = k.shadedHits; s.misses = k.misses; s.alphaTests = k.alphaTests;
  s.neeLookups = k.neeLookups; s.nodesVisited = k.nodesVisited; s.trisTested = k.trisTested;
  s.msGenerate = c->timers.ms[0]; s.msTraceClosest = c->timers.ms[1]; s.msShade = c->timers.ms[2]; s.msTraceShadow = c->timers.ms[3];
  s.msAccumulate = c->timers.ms[4];
  s.msTail       = c->timers.ms[5];
  s.launchesTraceClosest = c->timers.launchesClosest;
  s.launchesTail         = c->timers.launchesTail;
  s.msTraceFused         = c->timers.ms[6];
  s.launchesTraceFused   = c->timers.launchesFused;
  s.numMergedTriangles   = c->mergedTris;
  s.tailClosestRays = k.tailClosestRays; s.tailShadowRays = k.tailShadowRays; s.tailShadedHits = k.tailShadedHits; s.tailMisses = k.tailMisses;
  s.tailAlphaTests = k.tailAlphaTests;
  s.numTriangles = c->numTris;
  s.numBvhNodes  = PT_BVH_WIDTH == 2 ? c->numBvhNodes : c->numWideNodes;
  s.msBuildAccel = c->msBuild;
  s.numBlas      = c->numBlas;
  s.numTlasNodes = c->numTlasNodes;
  s.batchFrames    = uint32_t(c->batchMax);
  s.framesInFlight = uint32_t(c->inflight);
  s.bytesAccel   = c->dBvh.bytes + c->dWide.bytes + c->dTris.bytes + c->dAlphaRecs.bytes + c->dTlas.bytes + c->dTlasLeaves.bytes + c->dInstTriBase.bytes + c->dCNodes.bytes + c->dCTlas.bytes + c->dShadeTris.bytes;
  uint64_t bytes = 0;
  const DevBuf* sb[] = {&c->dVertices, &c->dIndices, &c->dInstances, &c->dMaterials, &c->dLights, &c->dTexRecs, &c->dTexels, &c->dBvh, &c->dWide, &c->dTris, &c->dAlphaRecs, &c->dAlphaMats, &c->dAlphaMaps, &c->dEnv, &c->dEnvAccel,
                        &c->dTlas, &c->dTlasLeaves, &c->dInstTriBase};
  for(const DevBuf* b : sb)
    bytes += b->bytes;
  s.bytesScene = bytes;
  *out         = s;
  return PT_OK;
}

int pt_reset_stats(pt_context* c)
{
  CTX_CHECK(c);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_all(c));
  pt_timers_collect(&c->timers);
  for(double& m : c->timers.ms)
    m = 0;
  c->timers.launchesClosest = 0;
  c->timers.launchesTail    = 0;
  c->timers.launchesFused   = 0;
  c->stats                  = pt_Stats{};
  HIP_TRY(c, hipMemset(c->dCounters.p, 0, sizeof(Counters)));
  clear_overflow(c);
  return PT_OK;
}

}  // extern "C"

