// The host build of the temporal stage: vk_raytrace_amd/csrc/pt_temporal.h compiled by g++, one whole call over row-major images in ordinary memory
// (stage/history_step.h).  tests/temporal_host.py compiles and binds it; tests/test_temporal_model.py holds it to a float64 model,
// tests/test_temporal_gpu.py holds the device to it.
#include "stage/history_step.h"

extern "C" {

// pt_temporal_accumulate on the host: the call's current frame and cameras, the history that is read (hist_colour == NULL for a first call) and whichever
// of the new history images and of the probe's outputs are asked for.  Returns what history_step returns; nothing is written on an error.
int th_temporal(const HistoryCall* q) { return q ? history_step(*q) : PT_ERR_INVALID; }

// temporal_constants: the status, and the static reason in why_out (why_len bytes, may be NULL)
int th_temporal_constants(const pt_TemporalParams* params, char* why_out, int why_len)
{
  const char* why = "";
  const int   rc  = temporal_constants(params, &why);
  copy_why(why, why_out, why_len);
  return rc;
}
}
