// pt_temporal_accumulate / pt_temporal_reset / pt_read_temporal_history (include/pt_api.h): the temporal reprojection stage of the display path
// (DESIGN.md section 5.3).  The per-pixel arithmetic is pt_temporal.h; this unit holds its kernel, the launch, the history the context keeps and the
// entry points.  No existing kernel is involved: the stage reads the row-major image the display pass already produces (untile_to_rowmajor), guide
// planes 1 and 2 and the camera, and writes only the history.
#include "pt_stage.h"
#include "pt_motion.h"  // (pt_temporal.h) the motion table of pt_temporal_accumulate_moving; its kernels are pt_motion.hip's
#include "pt_fast.h"    // the responsive history (section 5.7): its parameters and refusals; its kernel is pt_fast.hip's

// One block covers a TP_TX x TP_TY tile of the image, one pixel per lane: a wave covers two rows of 32 pixels, so that adjacent lanes read and write
// adjacent 16-byte pixels (512 contiguous bytes per row and plane) and the 4-byte length plane in 128-byte runs.  The gather is data dependent but
// coherent: neighbouring pixels reproject to neighbouring history positions.
#define TP_TX 32
#define TP_TY 8
#define TP_BLOCK (TP_TX * TP_TY)

struct TpArgs {
  const float4 *c, *g1, *g2;  // accumulation image (row-major), guide planes 1 and 2
  const float4 *hc, *hg;      // the history set that is read (never the set that is written: a lane gathers from positions other lanes write)
  const float*  hn;
  float4 *      hcOut, *hgOut;
  float*        hnOut;
  int           w, h;
  TemporalConst k;
};

struct TpGlobal {
  const TpArgs& a;
  __device__ size_t at(int x, int y) const { return size_t(y) * size_t(a.w) + size_t(x); }
  __device__ DnPx   colour(int x, int y) const { return stage_px(a.c[at(x, y)]); }
  __device__ DnPx   normal(int x, int y) const { return stage_px(a.g1[at(x, y)]); }
  __device__ DnPx   depth(int x, int y) const { return stage_px(a.g2[at(x, y)]); }
  __device__ DnPx   histColour(int x, int y) const { return stage_px(a.hc[at(x, y)]); }
  __device__ DnPx   histGuide(int x, int y) const { return stage_px(a.hg[at(x, y)]); }
  __device__ float  histLength(int x, int y) const { return a.hn[at(x, y)]; }
};

__global__ void __launch_bounds__(TP_BLOCK) k_temporal(TpArgs a)
{
  const int x = int(blockIdx.x) * TP_TX + int(threadIdx.x), y = int(blockIdx.y) * TP_TY + int(threadIdx.y);
  if(x >= a.w || y >= a.h)
    return;
  const TemporalOut o  = temporal_pixel(TpGlobal{a}, a.k, x, y, a.w, a.h, nullptr);
  const size_t      at = size_t(y) * size_t(a.w) + size_t(x);
  a.hcOut[at]          = make_float4(o.colour.x, o.colour.y, o.colour.z, o.colour.w);
  a.hgOut[at]          = make_float4(o.guide.x, o.guide.y, o.guide.z, o.guide.w);
  a.hnOut[at]          = o.length;
}

// The host-side record of one step: its images and its constants.  TpArgs above is k_temporal's kernel argument and is filled at that kernel's launch line only.
struct StepArgs {
  TemporalMArgs m;
  TemporalConst k;
};

// with the moments image (pt_temporal_track_moments) the kernel of pt_svgf.hip runs instead: the same pixel function, and the moments image besides.
// moving: the kernels of pt_motion.hip (section 5.5), over the instance plane and the table prepare_temporal uploaded (none without a history).
// demodulating (pt_temporal_demodulate): the kernels of pt_albedo.hip (section 5.6), which read guide plane 0 besides -- prepare_temporal saw to it.
static void launch_step(const pt_context* c, const StepArgs& s, bool moving)
{
  const TemporalMArgs& m     = s.m;
  const uint32_t*      ids   = (const uint32_t*)c->dInstPlane.p;
  const MotionRec*     table = (const MotionRec*)c->dMotionTable.p;
  const uint32_t       n     = moving && c->hist.have ? uint32_t(c->hInstances.size()) : 0u;  // (without a history there is no table)
  if(c->histSettings.demodulate)
    launch_temporal_d(c->stream, m, s.k, (const float4*)c->dGuide[0].p, moving, ids, table, n);
  else if(moving)
    launch_temporal_moving(c->stream, m, s.k, ids, table, n);
  else if(m.hmOut)
    launch_temporal_m(c->stream, m, s.k);
  else
    k_temporal<<<stage_grid(m.w, m.h, TP_TX, TP_TY), dim3(TP_TX, TP_TY), 0, c->stream>>>(TpArgs{m.c, m.g1, m.g2, m.hc, m.hg, m.hn, m.hcOut, m.hgOut, m.hnOut, m.w, m.h, s.k});
}

// The fast step's arguments (section 5.7), and the setting's constants in f: the long step's with the fast images in the place of Hc and Hn, maxFast in the place of
// maxHistory and no moments.  It reads (Hf, Hg, Hnf) of the set that is read and writes (Hf', Hnf'); Hg' is written again with the bits the long step gave it.
static StepArgs fast_step_args(const pt_context* c, const StepArgs& a, FastConst& f)
{
  const char* why = "";
  (void)fast_constants(&c->histSettings.fastParams, &f, &why);  // (pt_temporal_fast accepted them)
  const History& H = c->hist;
  StepArgs       b = a;
  b.m.hc           = (const float4*)H.fast[H.rd()].p;
  b.m.hn           = (const float*)H.fastLength[H.rd()].p;
  b.m.hm           = nullptr;
  b.m.hcOut        = (float4*)H.fast[H.wr()].p;
  b.m.hnOut        = (float*)H.fastLength[H.wr()].p;
  b.m.hmOut        = nullptr;
  b.k.maxHistory   = f.maxFast;
  return b;
}
static void enqueue_clamp(const pt_context* c, const StepArgs& a, const StepArgs& b, const FastConst& f)
{
  launch_fast_clamp(c->stream, b.m.hcOut, b.m.hnOut, a.m.hcOut, a.m.hnOut, a.m.w, a.m.h, f);
}

// One call's kernels, enqueued on the context's stream: the long step; with pt_temporal_fast on, the fast step -- the same kernel over other pointers,
// without moments -- and the clamp of what the long step wrote, in place, behind both.
static void launch_temporal(const pt_context* c, const StepArgs& a, bool moving = false)
{
  launch_step(c, a, moving);
  if(!c->histSettings.fast)
    return;
  FastConst      f{};
  const StepArgs b = fast_step_args(c, a, f);
  launch_step(c, b, moving);
  enqueue_clamp(c, a, b, f);
}

// the objectToWorld and worldToObject words of the scene's instances as they stand (none without a scene): what a call leaves with its history
static std::vector<float> instance_words(const pt_context* c)
{
  static_assert(sizeof(Affine) == 12 * sizeof(float) && offsetof(InstanceRec, worldToObject) == sizeof(Affine), "PT_MOTION_INSTANCE_WORDS words from the record's start");
  std::vector<float> words(c->haveScene ? c->hInstances.size() * PT_MOTION_INSTANCE_WORDS : 0);
  for(size_t i = 0; i * PT_MOTION_INSTANCE_WORDS < words.size(); ++i)
    std::memcpy(&words[i * PT_MOTION_INSTANCE_WORDS], &c->hInstances[i], PT_MOTION_INSTANCE_WORDS * sizeof(float));
  return words;
}

// Everything pt_temporal_accumulate checks, then both history sets allocated and the row-major accumulation image enqueued on the context's stream
// behind the frames rendered so far; the kernel's arguments in `a`.  Nothing of the history changes here.  moving: what the moving form needs besides,
// and its motion table made from the transforms kept with the history and the scene's current ones, on the device.
static int prepare_temporal(pt_context* c, const char* who, const pt_TemporalParams* p, StepArgs& a, bool moving = false)
{
  History& H = c->hist;
  STAGE_TRY(stage_need_image(c, who));
  if(!c->haveCamera)
    return c->fail(PT_ERR_STATE, "%s before pt_set_camera", who);
  if(!c->dGuide[1].p || !c->dGuide[2].p)
    return c->fail(PT_ERR_STATE, "%s: guide planes 1 (normal) and 2 (depth) must be installed (pt_render_guides or pt_set_denoise_guides)", who);
  const char* needs = "";
  if(albedo_step_needs_plane(c->histSettings.demodulate, guide_planes_set(c), &needs) != PT_OK)
    return c->fail(PT_ERR_STATE, "%s: %s", who, needs);
  STAGE_TRY(stage_need_full_image(c, who));
  const char* why = "";
  const int   rc  = temporal_constants(p, &why);
  if(rc != PT_OK)
    return c->fail(rc, "%s: %s", who, why);
  if(moving)
  {
    if(!c->dInstPlane.p)
      return c->fail(PT_ERR_STATE, "%s: no instance plane is installed (pt_render_instance_plane or pt_set_instance_plane)", who);
    if(!c->haveScene)
      return c->fail(PT_ERR_STATE, "%s before pt_set_scene", who);
    if(H.have && H.inst.size() != c->hInstances.size() * PT_MOTION_INSTANCE_WORDS)
      return c->fail(PT_ERR_STATE, "%s: the history was made with %zu instances, the scene has %zu (pt_temporal_reset)", who, H.inst.size() / PT_MOTION_INSTANCE_WORDS,
                     c->hInstances.size());
  }
  HIP_TRY(c, hipSetDevice(c->device));
  if(moving && H.have)
  {
    const std::vector<float> cur = instance_words(c);
    std::vector<MotionRec>   table(c->hInstances.size());
    motion_table(H.inst.data(), cur.data(), uint32_t(table.size()), table.data());
    STAGE_TRY(upload(c, c->dMotionTable, table.data(), sizeof(MotionRec) * table.size()));
  }
  STAGE_TRY(H.alloc(c, c->histSettings, stage_pixels(c)));
  STAGE_TRY(untile_to_rowmajor(c));
  const int  r = H.rd(), wr = H.wr();
  const bool mom = c->histSettings.trackMoments;
  a.m = TemporalMArgs{(const float4*)c->dRowMajor.p, (const float4*)c->dGuide[1].p, (const float4*)c->dGuide[2].p, (const float4*)H.colour[r].p, (const float4*)H.guide[r].p,
                      (const float*)H.length[r].p, mom ? (const float2*)H.moments[r].p : nullptr, (float4*)H.colour[wr].p, (float4*)H.guide[wr].p,
                      (float*)H.length[wr].p, mom ? (float2*)H.moments[wr].p : nullptr, c->width, c->height};
  a.k = temporal_const(c->scene.camera.viewInverse, c->scene.camera.projInverse, H.have ? H.worldToClip : nullptr, H.have ? H.eye : nullptr, p);
  return PT_OK;
}

// one call of either form
static int temporal_accumulate(pt_context* c, const char* who, const pt_TemporalParams* p, float* out, bool moving)
{
  StepArgs a;
  STAGE_TRY(prepare_temporal(c, who, p, a, moving));
  launch_temporal(c, a, moving);
  HIP_TRY(c, hipGetLastError());
  if(out)
    HIP_TRY(c, hipMemcpyAsync(out, a.m.hcOut, sizeof(float4) * stage_pixels(c), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, sync_all(c));
  c->hist.commit(c->histSettings, p->worldToClip, &c->scene.camera.viewInverse[12], instance_words(c));
  return check_traversal(c);
}

extern "C" {

int pt_temporal_accumulate(pt_context* c, const pt_TemporalParams* p, float* out)
{
  CTX_CHECK(c);
  return temporal_accumulate(c, "pt_temporal_accumulate", p, out, false);
}

int pt_temporal_accumulate_moving(pt_context* c, const pt_TemporalParams* p, float* out)
{
  CTX_CHECK(c);
  return temporal_accumulate(c, "pt_temporal_accumulate_moving", p, out, true);
}

int pt_temporal_reset(pt_context* c)
{
  CTX_CHECK(c);
  c->hist.drop();  // the buffers stay for the next call; pt_resize and pt_destroy free them
  return PT_OK;
}

int pt_temporal_track_moments(pt_context* c, int on)
{
  CTX_CHECK(c);
  if(on != 0 && on != 1)
    return c->fail(PT_ERR_INVALID, "pt_temporal_track_moments: on must be 0 or 1");
  c->hist.set_to(c->histSettings.trackMoments, on != 0);  // a history without moments cannot be continued with them, and the other way round
  return PT_OK;
}

int pt_temporal_demodulate(pt_context* c, int on)
{
  CTX_CHECK(c);
  const char* why = "";
  if(albedo_setting(on, &why) != PT_OK)
    return c->fail(PT_ERR_INVALID, "pt_temporal_demodulate: %s", why);
  c->hist.set_to(c->histSettings.demodulate, on != 0);  // a history of colour cannot be continued with illumination, and the other way round
  return PT_OK;
}

int pt_temporal_fast(pt_context* c, const pt_FastParams* p)
{
  CTX_CHECK(c);
  if(p)
  {
    const char* why = "";
    const int   rc  = fast_constants(p, nullptr, &why);
    if(rc != PT_OK)
      return c->fail(rc, "pt_temporal_fast: %s", why);
    c->histSettings.fastParams = *p;  // new parameters while the setting stays on keep the history
  }
  c->hist.set_to(c->histSettings.fast, p != nullptr);  // a history without the fast images cannot be continued with them, and the other way round
  return PT_OK;
}

int pt_read_temporal_fast(pt_context* c, float* rgba32f_out, float* length_out)
{
  CTX_CHECK(c);
  STAGE_TRY(stage_need_history(c, "pt_read_temporal_fast", false));
  const char* why = "";
  if(fast_need_history(c->hist.isFast, &why) != PT_OK)
    return c->fail(PT_ERR_STATE, "pt_read_temporal_fast: %s", why);
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n = stage_pixels(c);
  return stage_read(c, {{rgba32f_out, c->hist.fast[c->hist.rd()].p, sizeof(float4) * n}, {length_out, c->hist.fastLength[c->hist.rd()].p, sizeof(float) * n}});
}

int pt_read_temporal_history(pt_context* c, float* rgba32f_out, float* length_out)
{
  CTX_CHECK(c);
  STAGE_TRY(stage_need_history(c, "pt_read_temporal_history", false));
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n = stage_pixels(c);
  return stage_read(c, {{rgba32f_out, c->hist.colour[c->hist.rd()].p, sizeof(float4) * n}, {length_out, c->hist.length[c->hist.rd()].p, sizeof(float) * n}});
}

// Measurement access (not part of pt_api.h; tools/temporal_rate.py): the kernel of pt_temporal_accumulate enqueued `reps` times between two events on
// the context's stream, after one untimed run -- milliseconds per run in *ms_out, without the untile pass before it and without any copy.  Every run
// reads the history and writes the other set; the history itself stays as it was.  Synchronous.
__attribute__((visibility("default"))) int pt_debug_temporal_time(pt_context* c, const pt_TemporalParams* p, int reps, float* ms_out)
{
  CTX_CHECK(c);
  if(!ms_out || reps < 1)
    return c->fail(PT_ERR_INVALID, "pt_debug_temporal_time: null or reps < 1");
  StepArgs a;
  STAGE_TRY(prepare_temporal(c, "pt_debug_temporal_time", p, a));
  return stage_time(c, "pt_debug_temporal_time", reps, ms_out, [&] { launch_temporal(c, a); });  // (the kernel the setting of pt_temporal_track_moments selects)
}

// Measurement access (not part of pt_api.h; tools/motion_rate.py).  what = 0: the pass of pt_render_instance_plane(planes, miss_depth), timed as
// pt_debug_guides_time times the guide pass (params is not read); what = 1: the kernel of pt_temporal_accumulate_moving, timed as pt_debug_temporal_time
// times pt_temporal_accumulate's, with the motion table of the current instance transforms against the history's.  Synchronous.
__attribute__((visibility("default"))) int pt_debug_motion_time(pt_context* c, const pt_TemporalParams* p, int what, uint32_t planes, float miss_depth, int reps, float* ms_out)
{
  CTX_CHECK(c);
  if(!ms_out || reps < 1 || (what != 0 && what != 1))
    return c->fail(PT_ERR_INVALID, "pt_debug_motion_time: null, reps < 1 or no such part");
  if(what == 0)
    return debug_instances_time(c, planes, miss_depth, reps, ms_out);
  StepArgs a;
  STAGE_TRY(prepare_temporal(c, "pt_debug_motion_time", p, a, true));
  return stage_time(c, "pt_debug_motion_time", reps, ms_out, [&] { launch_temporal(c, a, true); });
}

// Measurement access (not part of pt_api.h; tools/albedo_rate.py).  what = 0: the demodulating temporal kernel the settings select (pt_temporal_demodulate
// must be on; the static form, with or without the moments as pt_temporal_track_moments says), timed as pt_debug_temporal_time times
// pt_temporal_accumulate's; what = 1: the remodulation pass over one image (params is not read).  Synchronous.
__attribute__((visibility("default"))) int pt_debug_albedo_time(pt_context* c, const pt_TemporalParams* p, int what, int reps, float* ms_out)
{
  CTX_CHECK(c);
  if(!ms_out || reps < 1 || (what != 0 && what != 1))
    return c->fail(PT_ERR_INVALID, "pt_debug_albedo_time: null, reps < 1 or no such part");
  if(what == 1)
    return debug_remodulate_time(c, reps, ms_out);
  if(!c->histSettings.demodulate)
    return c->fail(PT_ERR_STATE, "pt_debug_albedo_time: pt_temporal_demodulate is off");
  StepArgs a;
  STAGE_TRY(prepare_temporal(c, "pt_debug_albedo_time", p, a));
  return stage_time(c, "pt_debug_albedo_time", reps, ms_out, [&] { launch_temporal(c, a); });
}

// Measurement access (not part of pt_api.h; tools/fast_rate.py), with pt_temporal_fast on and a history made that way.  what = 0: the fast step -- the
// temporal kernel the other settings select, without moments, over the fast images; what = 1: k_fast_clamp with the setting's parameters.  Before the
// timed runs the whole call's kernels run once, untimed, so that the clamp finds what a call gives it; every run writes the set that is not the history,
// which stays as it was.  Synchronous.
__attribute__((visibility("default"))) int pt_debug_fast_time(pt_context* c, const pt_TemporalParams* p, int what, int reps, float* ms_out)
{
  CTX_CHECK(c);
  if(!ms_out || reps < 1 || (what != 0 && what != 1))
    return c->fail(PT_ERR_INVALID, "pt_debug_fast_time: null, reps < 1 or no such part");
  if(!c->histSettings.fast)
    return c->fail(PT_ERR_STATE, "pt_debug_fast_time: pt_temporal_fast is off");
  STAGE_TRY(stage_need_history(c, "pt_debug_fast_time", false));
  StepArgs a;
  STAGE_TRY(prepare_temporal(c, "pt_debug_fast_time", p, a));
  FastConst      f{};
  const StepArgs b = fast_step_args(c, a, f);
  return stage_time(c, "pt_debug_fast_time", reps, ms_out, [&] { what == 0 ? launch_step(c, b, false) : enqueue_clamp(c, a, b, f); }, [&] { launch_temporal(c, a); });
}

}  // extern "C"
