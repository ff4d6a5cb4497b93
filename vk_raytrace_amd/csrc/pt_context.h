// The context behind the C ABI (include/pt_api.h) and the few helpers its translation units share.  Internal: not installed.
// pt_capi.hip defines the helpers; pt_capi_accel.hip (acceleration structures) and pt_debug.hip (calibration and test kernels) use them.
#pragma once
#include <cstdarg>
#include <cstdio>
#include "../../include/pt_api.h"
#include "pt_internal.h"  // (hip_runtime.h, <string>, <vector>)

struct DevBuf {
  void*  p     = nullptr;
  size_t bytes = 0;
};
struct pt_context;
// device memory (pt_capi.hip).  dev_alloc keeps a buffer that is large enough and at most twice too large; upload = dev_alloc + copy.
int  dev_alloc(pt_context* c, DevBuf& b, size_t bytes);
bool dev_alloc_quiet(DevBuf& b, size_t bytes);  // like dev_alloc, but a failed allocation is an answer (false), not an error
void dev_free(DevBuf& b);
int  upload(pt_context* c, DevBuf& b, const void* src, size_t bytes);
#include "pt_history.h"  // History, HistorySettings: members of the context

struct pt_context {
  PtTuning    tune;  // launch-policy knobs of THIS context (PT_TUNE at pt_create)
  int         device = 0;
  hipStream_t stream = nullptr;
  std::string err;

  // scene (host copies kept only for what build_accel needs)
  DevBuf   dMatLines;  // one 128-byte line per material (DeviceScene::matLines)
  DevBuf   dVertices, dIndices, dInstances, dMaterials, dLights, dTexRecs, dTexels, dBvh, dWide, dTris, dAlphaRecs, dAlphaMats, dAlphaMaps, dEnv, dEnvAccel;
  DevBuf   dShadeTris;
  bool     haveShadeTris = false;
  DevBuf   dInstBlock;  // DeviceScene::instBlock
  DevBuf   dCTlas;   // DeviceScene::ctlas
  std::vector<uint32_t> hBlasRanges;  // two-level mode: (node base, wide nodes) of every object-space BLAS
  uint32_t nodeCapacity = 0;          // nodes dWide was sized for (two-level mode: the BLASes sit at their node bases)
  DevBuf   dCNodes;  // DeviceScene::cnodes (flat-format structures, PT_TUNE cnodes=1)
  bool     haveCNodes = false;
  uint32_t numTris = 0, numInstances = 0, numBvhNodes = 0, numWideNodes = 0, numLights = 0;
  // two-level acceleration structure (pt_set_accel_mode): dWide / dTris / dAlphaRecs hold the concatenated BLASes, dTlas the instance hierarchy
  int      accelMode = PT_ACCEL_FLAT;
  DevBuf   dTlas, dTlasLeaves, dInstTriBase, dActive, dInstNodeBase, dInstPad;
  uint32_t numBlas = 0, numTlasNodes = 0, numActive = 0;
  // two-level mode: the instances whose prim-mesh is instantiated exactly once live in one world-space structure (PT_INST_MERGED) at slot 0 /
  // node 0 of the BLAS arrays; mergedOnly: nothing else exists, the structure IS the flat one and the flat kernels run on it
  std::vector<uint32_t> hMerged;
  uint32_t mergedTris = 0, mergedWide = 0;
  float    mergedBox[6] = {0, 0, 0, 0, 0, 0};
  bool     mergedOnly = false;
  std::vector<uint32_t> hInstNodeBase;  // per instance: root node of its BLAS (two-level mode, after the BLAS build)
  std::vector<float>    hPrimBound;     // per prim-mesh: max |coordinate| of its vertices (object space); bounds the rounding of the ray transform
  // deforming meshes (pt_update_vertices / pt_refit_accel)
  uint32_t numVertices = 0;
  std::vector<uint32_t> hPrimMeshVerts;  // per prim-mesh: (vertexOffset, vertexCount), from pt_set_scene
  std::vector<float>    hPositions;      // the positions of the vertex buffer, three floats per vertex: hPrimBound of a touched mesh is made again from them
  std::vector<char>     primTouched;     // per prim-mesh: a vertex of it changed since hPrimBound was computed
  std::vector<PtBlasDesc> hBlas;         // two-level mode: the object-space BLASes as built (slot and node bases, mesh)
  bool     accelStale = false;           // a structure exists and pt_update_vertices changed vertices since: haveAccel is false until a refit or a build
  DevBuf   dRefit;                       // the parent table of the current build (pt_refit.hip), made by the first refit after it
#if PT_BVH_WIDTH == 4
  PtRefitTable refit;
#endif
  bool     haveRefitTable = false;
  // tree cost of the structure as built (pt_RefitInfo::costBefore = their sum): [0] the flat or merged hierarchy, [1] the BLASes.  Measured when the parent
  // table is made; the BLASes' part is kept when only the merged structure is built again (pt_update_instances), because by then a refit may have changed them
  double   costBuilt[2] = {0, 0};
  bool     haveCostBlas = false;
  // why a call that walks the structure is refused
  const char* no_accel() const { return accelStale ? "with a refit pending (pt_update_vertices changed the vertices: call pt_refit_accel or pt_build_accel first)" : "before pt_set_scene / pt_build_accel"; }
  double   msBuildTlas = 0;
  bool     renderedSinceCheck = false;  // frames were launched since the traversal-stack overflow counter was last looked at
  unsigned overflowSeen = 0;           // traversal-stack overflows counted so far (check_traversal); cleared with the counters
  bool     anyHit = true;               // RtxPipeline::useAnyHit (src/rtx_pipeline.cpp:269-276); false: every triangle is opaque
  std::vector<InstanceRec> hInstances;  // as built by pt_set_scene (flags without the useAnyHit override)
  bool     haveScene = false, haveAccel = false, haveEnv = false, haveCamera = false;
  bool     warmPending = true;  // the next pt_resize warms the frame slots (once per acceleration structure: not on the resizes of an interactive session)
  DeviceScene scene{};

  // output / path state
  int      width = 0, height = 0, tilesX = 0, tilesY = 0;
  int      rank = 0, nranks = 1;
  uint32_t numLocalTiles = 0, maxTilesPerRank = 0, numSlots = 0;
  uint64_t localPixels = 0;
  // Frames in flight: each has its own path state, queues, counter block and stream, so that the long tail of one
  // frame's stage (a launch lasts as long as its slowest ray) is filled with the work of other frames.  Only the
  // running-mean accumulate is ordered across frames (events).
  struct __attribute__((visibility("hidden"))) FrameSlot {  // (pt_api.h names pt_context inside its exported region: the members are not ABI)
    // per path: 9 float4 arrays of path state and 6 queues of path-slot indices.  bind() is the only place that says which is which.
    DevBuf        dState[9], dQueue[6], dCounts, dCountsDone;
    RenderBuffers rb{};
    hipStream_t   stream    = nullptr;
    hipEvent_t    accumDone = nullptr;
    bool          launched  = false;  // a launch sequence was enqueued on this slot since the last synchronisation
    // queue-size feedback: the per-bounce counters of the slot's latest launch sequence come back asynchronously (pinned memory)
    uint32_t*     hCounts     = nullptr;
    hipEvent_t    countsDone  = nullptr;
    uint64_t      countsSeq   = 0;   // sequence number of the launch the copy belongs to (0: none)
    uint32_t      countsPaths = 0;   // paths of that launch (frames of the batch x local pixels)
    int           countsDepths = 0;  // bounces it ran staged (the counters of later bounces are not produced: k_tail took over)

    static constexpr size_t bytesPerPath = 9 * sizeof(float4) + 6 * sizeof(uint32_t);
    // f(buffer, bytes per path) for every buffer whose size follows the number of paths
    template <class F>
    void each_path_buffer(F&& f)
    {
      for(DevBuf& b : dState)
        f(b, sizeof(float4));
      for(DevBuf& b : dQueue)
        f(b, sizeof(uint32_t));
    }
    size_t     bytes_held();
    bool       alloc(size_t paths);  // path buffers for `paths` paths and the two counter blocks; false: out of device memory
    hipError_t clear_counts();       // a sample pass starts on a cleared counter block: cleared by pt_resize once, then by every k_accumulate
    void       release_paths();
    void       bind(float4* frame, uint32_t* slotTile, Counters* counters);  // fills rb from the buffers
  };
  FrameSlot slots[PT_MAX_INFLIGHT];
  int       inflight     = 1;  // frame slots in use (<= inflightMax: pt_resize drops slots when the device memory is short)
  int       inflightMax  = 1;  // frame slots created (streams / events exist for these)
  // Display slots: slots[inflightMax .. inflightMax + displaySlots) hold the path state of ONE frame each and join the ring only for launches of a
  // single frame -- the display loop (render, tonemap, present per frame), where six short sequences in flight beat four by 12 %, while batches
  // are fastest on four full slots (profiles/r04y_display_slots.txt)
  int       displaySlots    = 0;  // in use after pt_resize
  int       displaySlotsMax = 0;  // created
  uint64_t  displayCounter  = 0;  // ring position of the single-frame launches
  // frames handed to pt_render_frame but not launched yet: consecutive frames with identical state are traced as one
  // batch (flushed when full and by every call that reads results or changes inputs)
  pt_RtxState pendState{};
  int         pendCount = 0;
  int         batchMax  = 1;
  int         variant   = PT_VARIANT_RAYQUERY;
  uint64_t  frameCounter = 0;
  // fraction of a launch's paths still alive at the start of bounce d, from the most recent finished launch (queue-size feedback; decides
  // where k_tail takes over -- performance only)
  double    qRatio[PT_MAX_DEPTH + 1];
  int       qRatioDepths = 0;   // entries of qRatio that were observed (0: nothing observed yet)
  uint64_t  qRatioSeq    = 0;   // launch they come from
  uint64_t  launchSeq    = 0;
  hipEvent_t lastAccum   = nullptr;  // accumDone of the most recent frame (nullptr: none pending)
  DevBuf   dFrame, dSlotTile, dCounters;
  DevBuf   dPick;
  DevBuf   dQueryRays, dQueryHits;  // pt_trace_rays with host arrays: staging buffers of PT_QUERY_CHUNK records each, allocated on first use
  DevBuf   dPathsChunk;             // pt_trace_paths (pt_paths.hip): the word its wavefronts reserve rays from, cleared on the stream before each launch
  int      pathsWaves = 0;          // wavefronts of its launches (0: the default; pt_debug_paths_waves)
  DevBuf   dPointsChunk;            // pt_gather (pt_gather.hip): the word its wavefronts reserve points from, cleared on the stream before each launch
  int      pointsWaves = 0;         // wavefronts of its launches (0: the default; pt_debug_gather_waves)
  DevBuf   dRowMajor, dRgba8, dMean, dMips, dGather, dFullTiles, dFullSlotTile, dTileLocalIndex;
  // denoiser (pt_denoise.hip): the two ping-pong images, allocated on first use, and the caller's guide planes; pt_resize and pt_destroy free them
  DevBuf   dDenoise[2], dGuide[PT_DENOISE_GUIDES];
  int      denoiseLdsMaxStep = -1;  // largest step whose iteration stages its tile in LDS (-1: the measured default; pt_debug_denoise_lds)
  History         hist;          // the history of the display path (pt_history.h; pt_temporal.hip writes it) ...
  HistorySettings histSettings;  // ... and the settings the next temporal call runs under
  // motion of moving instances (pt_motion.hip): the instance plane (one word per pixel) and the motion table of the call in flight
  DevBuf   dInstPlane, dMotionTable;
  DevBuf   dChainPlane;  // the link plane of the chained guide pass (pt_chain.hip): one word per pixel
  // variance-guided filter (pt_svgf.hip): the filter's two variance planes, allocated on first use
  DevBuf   dSvgfVar[2];
  int      svgfLdsMaxStep = -1;  // largest step whose iteration stages its tile in LDS (-1: the measured default; pt_debug_svgf_lds)
  bool     haveFull = false;
  // pipelined display (pt_tonemap_begin / pt_tonemap_end): a ring of pinned host images, each with the event that says its copy has landed
  // and the event after which the accumulation image may be written again (the untile pass has read it)
  struct DisplaySlot {
    uint8_t*   host  = nullptr;
    size_t     bytes = 0, used = 0;
    hipEvent_t done = nullptr, read = nullptr;
    unsigned*  overflow = nullptr;  // pinned: the overflow counter as the display pass saw it (pt_tonemap_end reports it)
  };
  DisplaySlot display[PT_DISPLAY_RING];
  uint64_t    displayHead = 0, displayTail = 0;  // oldest image not collected yet / next one to fill
  bool     gatherEnqueued = false;  // pt_gather_shards ran on this context as the root and pt_gather_finish has not consumed it yet
  StageTimers timers;
  pt_Stats    stats{};
  double      msBuild = 0;

  int fail(int code, const char* fmt, ...)
  {
    char    buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    if(code == PT_ERR_HIP)
      countsDirty = true;  // a launch sequence may have died before its k_accumulate cleared the per-bounce counters: flush_pending repairs them first
    return code;
  }
  bool countsDirty = false;
};

#define CTX_CHECK(ctx)       \
  if(!(ctx))                 \
    return PT_ERR_INVALID;
#define HIP_TRY(ctx, call)                                                                                   \
  do                                                                                                         \
  {                                                                                                          \
    hipError_t e_ = (call);                                                                                  \
    if(e_ != hipSuccess)                                                                                     \
      return (ctx)->fail(e_ == hipErrorOutOfMemory ? PT_ERR_OOM : PT_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
  } while(0)

// shared by the units of the ABI, defined in pt_capi.hip (hidden like everything that pt_api.h does not name)
int        flush_pending(pt_context* c);    // launches the frames handed to pt_render_frame that have not been launched yet
hipError_t sync_all(pt_context* c);         // flush_pending, then waits for every stream of the context
int        check_traversal(pt_context* c);  // after a synchronisation: PT_ERR_STATE once a traversal ran out of stack
void       clear_overflow(pt_context* c);
int        untile_to_rowmajor(pt_context* c);  // the row-major accumulation image in dRowMajor, enqueued behind the frames rendered so far
int        display_chain(pt_context* c, int dispW, int dispH, bool chain, hipEvent_t readDone, MipView& mv);  // the display pass's offscreen image and its mip chain, enqueued
int        display_levels(pt_context* c, const float4* image, int dispW, int dispH, bool chain, MipView& mv);  // ... the part after level 0 (`image`, accumulation size) is chosen
int        display_finish(pt_context* c, const pt_Tonemapper* tm, MipView& mv, int dispW, int dispH, uint8_t* out);  // ... the tonemap kernel and the copy to `out` (host), enqueued
// everything a query through the path loop checks before it launches (pt_paths.hip; pt_trace_paths and pt_gather, DESIGN.md sections 3.2 / 3.3),
// each refusal with its own text under the caller's name `who`; then the kernel's parameters filled.  Nothing is allocated or launched.
int        path_query_checks(pt_context* c, const char* who, const pt_RtxState* st, uint32_t flags, uint64_t n, const void* in, const void* results, FrameParams& fp);
void       refresh_scene_ptrs(pt_context* c);
int        upload_instances(pt_context* c);
std::vector<InstanceRec> effective_instances(const pt_context* c);  // the instance records as the kernels see them
