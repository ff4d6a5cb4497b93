// The history of the display path as a context keeps it (DESIGN.md sections 5.3 - 5.7): its buffers, what it was made with, the settings the next call
// runs under, and the only functions that change any of it.  pt_temporal.hip writes it; pt_svgf.hip, pt_denoise.hip and pt_stage.h read it.  Below them,
// what the temporal step launches from other units.  Host code.  Internal: not installed.  pt_context.h includes it, after DevBuf and dev_alloc.
#pragma once
#include <algorithm>

// what pt_temporal_track_moments, pt_temporal_demodulate and pt_temporal_fast set: how the next call makes its history
struct HistorySettings {
  bool          trackMoments = false;  // the history has a fourth image, the luminance moments (pt_svgf.hip)
  bool          demodulate   = false;  // the step divides the pixel's own colour by guide plane 0 (pt_albedo.hip, section 5.6)
  bool          fast         = false;  // the step keeps a second, short history and clamps the long one to it (pt_fast.hip, section 5.7)
  pt_FastParams fastParams   = {};
};

struct History {
  // colour, packed guide (encoded normal, depth), length; the moments (float2); the fast colour and length, which share the guide image.  Each twice: one
  // set is read while the other is written.  Allocated on first use (alloc), freed by pt_resize and pt_destroy (release); drop() keeps them.
  DevBuf colour[2], guide[2], length[2], moments[2], fast[2], fastLength[2];
  int    set  = 0;      // the set that holds the history: the next call reads it and writes the other
  bool   have = false;  // false: first call, or dropped -- no pixel has history
  // the settings the held history was made with: its consumers need the moments, multiply their final image by guide plane 0, read the fast images
  bool  hasMoments = false, demodulated = false, isFast = false;
  float worldToClip[16] = {0}, eye[3] = {0, 0, 0};  // the camera it was made with
  std::vector<float> inst;  // objectToWorld and worldToObject of every instance as they were then (24 words each, section 5.5)

  int rd() const { return set; }
  int wr() const { return set ^ 1; }
  // the one place the history is dropped: the buffers stay for the next call
  void drop() { have = hasMoments = demodulated = isFast = false; }
  void release()
  {
    for(DevBuf(*b)[2] : {&colour, &guide, &length, &moments, &fast, &fastLength})
      dev_free((*b)[0]), dev_free((*b)[1]);
    drop();
  }
  // both sets of every image the settings ask for, for n pixels
  int alloc(pt_context* c, const HistorySettings& s, size_t n)
  {
    const struct { DevBuf (&b)[2]; size_t bytes; bool wanted; } images[] = {{colour, 16 * n, true},           {guide, 16 * n, true},  {length, 4 * n, true},
                                                                            {moments, 8 * n, s.trackMoments}, {fast, 16 * n, s.fast}, {fastLength, 4 * n, s.fast}};
    for(const auto& im : images)
      for(int i = 0; i < 2 && im.wanted; ++i)
        if(const int rc = dev_alloc(c, im.b[i], im.bytes))
          return rc;
    return PT_OK;
  }
  // the set just written is the history now, made with this camera, these settings and these instance transforms
  void commit(const HistorySettings& s, const float* worldToClipNow, const float* eyeNow, std::vector<float> instNow)
  {
    std::copy(worldToClipNow, worldToClipNow + 16, worldToClip);
    std::copy(eyeNow, eyeNow + 3, eye);
    inst = std::move(instNow);
    set ^= 1;
    have = true;
    hasMoments = s.trackMoments, demodulated = s.demodulate, isFast = s.fast;  // (demodulated: what the history holds is illumination then)
  }
  // behind the three setting entry points: a history made under one value cannot be continued under the other, the same value again keeps it
  void set_to(bool& setting, bool value)
  {
    if(setting != value)
      drop();
    setting = value;
  }
};

// ---- what a temporal step launches from the other units -------------------------------------------------------------------------------------------------
struct TemporalConst; struct MotionRec; struct FastConst;  // (pt_temporal.h, pt_motion.h, pt_fast.h)
struct TemporalMArgs {  // the host-side record of a step's images, and a member of the kernel arguments of pt_svgf.hip, pt_motion.hip and pt_albedo.hip
  const float4 *c, *g1, *g2, *hc, *hg;
  const float*  hn;
  const float2* hm;
  float4 *      hcOut, *hgOut;
  float*        hnOut;
  float2*       hmOut;  // hm / hmOut NULL: a step without the moments image
  int           w, h;
};
// pt_svgf.hip: k_temporal_m, the temporal kernel that also writes the moments
void launch_temporal_m(hipStream_t stream, const TemporalMArgs& a, const TemporalConst& k);
// pt_motion.hip: the temporal kernels of pt_temporal_accumulate_moving (a.hm == NULL: the one without the moments image) and the timing of its instance pass
void launch_temporal_moving(hipStream_t stream, const TemporalMArgs& a, const TemporalConst& k, const uint32_t* ids, const MotionRec* table, uint32_t numInstances);
int  debug_instances_time(pt_context* c, uint32_t planes, float missDepth, int reps, float* ms_out);
// pt_albedo.hip: the temporal kernels of a context with pt_temporal_demodulate on (a.hm == NULL: without the moments image; ids / table / numInstances
// are read by the moving form only), the remodulation of n pixels (out may be c) and the timing of that pass
void launch_temporal_d(hipStream_t stream, const TemporalMArgs& a, const TemporalConst& k, const float4* albedo, bool moving, const uint32_t* ids, const MotionRec* table,
                       uint32_t numInstances);
void launch_remodulate(hipStream_t stream, const float4* albedo, const float4* c, float4* out, size_t n);
int  debug_remodulate_time(pt_context* c, int reps, float* ms_out);
// pt_fast.hip: the clamp of the long history that was just written (hc, hn: in place, each lane its own pixel) to the fast one written beside it (hf, hnf)
void launch_fast_clamp(hipStream_t stream, const float4* hf, const float* hnf, float4* hc, float* hn, int w, int h, const FastConst& k);
