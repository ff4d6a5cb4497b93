// The counters of the T2 experiments (t2_variants.h), read and cleared: part of the "robust" and "certified" flavours of the harness only.
#include "../th_shims.h"

extern "C" void th_t2_stats(unsigned long long* out2) { out2[0] = g_t2Calls.exchange(0); out2[1] = g_t2Double.exchange(0); }
#ifdef TH_CERTIFIED_T2
extern "C" unsigned long long th_t2_accepts() { return g_t2Accepts.exchange(0); }
#endif
