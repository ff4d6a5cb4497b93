// The product's functions one call at a time (unit of the host harness, tests/host_harness.py): the four probes of pt_probe.h and the records a
// scene made by th_create_scene holds.  The device runs the same functions per lane (pt_debug_*_probe).
#include "th_scene.h"
#include "pt_probe.h"  // shading_probe, texture_probe, surface_probe, trace_probe: one call of a product function per row

extern "C" {

// ---- the shading functions one at a time (pt_probe.h): BSDF evaluation / sampling, sun & sky, environment uv, tangent frame, punctual-light
// attenuation, the GLSL built-ins of pt_math.h -- n states, one row each.  The device runs the same function per lane (pt_debug_shading_probe).
int th_shading_probe(int fn, uint64_t n, const float* in, int in_stride, float* out, int out_stride)
{
  int inWords = 0, outWords = 0;
  probe_row_words(fn, inWords, outWords);
  if(inWords == 0 || in_stride < inWords || out_stride < outWords)
    return -1;
#pragma omp parallel for schedule(static)
  for(long long i = 0; i < (long long)n; ++i)
    shading_probe(fn, in + size_t(i) * in_stride, out + size_t(i) * out_stride);
  return 0;
}

// ---- the software texture path one call at a time (pt_probe.h texture_probe) on a scene made by th_create_scene: the product's own records, material
// lines, opacity maps and pool (pt_debug_scene_records), the environment of th_set_env.  The device runs the same function per lane (pt_debug_texture_probe).
int th_texture_probe(void* p, int kind, uint64_t n, const float* in, int in_stride, float* out, int out_stride)
{
  Scene* s = static_cast<Scene*>(p);
  if(!s || kind < 0 || kind >= TEXP_COUNT || in_stride < TEXP_IN || out_stride < TEXP_OUT)
    return -1;
  const TexProbeLimits lim{uint32_t(s->texRecs.size()), uint32_t(s->alphaMats.size() < s->matLines.size() / PT_MAT_LINE_QUADS ? s->alphaMats.size() : s->matLines.size() / PT_MAT_LINE_QUADS),
                           uint32_t(s->texels.size())};
#pragma omp parallel for schedule(static)
  for(long long i = 0; i < (long long)n; ++i)
    texture_probe(s->dsFlat, lim, kind, in + size_t(i) * in_stride, out + size_t(i) * out_stride);
  return 0;
}
// ---- a hit turned into a Surface (pt_probe.h surface_probe) on a scene made by th_create_scene: its instance records, packed vertices, indices, materials,
// material lines and pool.  The device runs the same function per lane (pt_debug_surface_probe).  Returns SURF_NO_DATA (1) for SURF_SLOT: the host build keeps
// no per-slot shading lines.
int th_surface_probe(void* p, int kind, uint64_t n, const float* in, int in_stride, float* out, int out_stride)
{
  Scene* s = static_cast<Scene*>(p);
  if(!s || kind < 0 || kind >= SURF_COUNT || in_stride < SURF_IN || out_stride < SURF_OUT)
    return -1;
  if(kind == SURF_SLOT && s->dsFlat.shadeTris == nullptr)
    return SURF_NO_DATA;
  const size_t          mats = s->materials.size() < s->matLines.size() / PT_MAT_LINE_QUADS ? s->materials.size() : s->matLines.size() / PT_MAT_LINE_QUADS;
  const SurfProbeLimits lim{uint32_t(s->inst.size()), uint32_t(s->indices.size()), uint32_t(s->vertices.size() / 2), uint32_t(mats), uint32_t(s->texRecs.size()),
                            uint32_t(s->texels.size()), 0u};
#pragma omp parallel for schedule(static)
  for(long long i = 0; i < (long long)n; ++i)
    (void)surface_probe(s->dsFlat, lim, kind, in + size_t(i) * in_stride, out + size_t(i) * out_stride);
  return 0;
}
// ---- the intersection arithmetic one call at a time (pt_probe.h trace_probe): n rows, each read and written in place.  The device runs the same function per
// lane (pt_debug_trace_probe).
int th_trace_probe(int kind, uint64_t n, const float* in, int in_stride, float* out, int out_stride)
{
  int inWords = 0, outWords = 0;
  trace_row_words(kind, inWords, outWords);
  if(inWords == 0 || in_stride < inWords || out_stride < outWords)
    return -1;
#pragma omp parallel for schedule(static)
  for(long long i = 0; i < (long long)n; ++i)
  {
    float row[TRP_IN], res[TRP_OUT];
    for(int k = 0; k < TRP_IN; ++k)
      row[k] = k < inWords ? in[size_t(i) * in_stride + k] : 0.0f;
    for(int k = 0; k < TRP_OUT; ++k)
      res[k] = k < outWords ? out[size_t(i) * out_stride + k] : 0.0f;
    trace_probe(kind, row, res);
    std::memcpy(out + size_t(i) * out_stride, res, sizeof(float) * size_t(outWords));
  }
  return 0;
}
// the scene's texture records (TexRec, 32 B each), material lines (PT_MAT_LINE_QUADS x 16 B per material), alpha view (AlphaMat, 80 B each), opacity maps
// and texel pool as th_create_scene fetched them; null outputs: the counts only (records, materials, map words, pool texels)
void th_texture_records(void* p, unsigned long long* counts4, void* texRecsOut, void* matLinesOut, void* alphaMatsOut, uint32_t* alphaMapsOut, uint32_t* texelsOut)
{
  Scene* s = static_cast<Scene*>(p);
  counts4[0] = s->texRecs.size(); counts4[1] = s->matLines.size() / PT_MAT_LINE_QUADS; counts4[2] = s->alphaMaps.size(); counts4[3] = s->texels.size();
  if(texRecsOut) std::memcpy(texRecsOut, s->texRecs.data(), sizeof(TexRec) * s->texRecs.size());
  if(matLinesOut) std::memcpy(matLinesOut, s->matLines.data(), sizeof(uint4) * s->matLines.size());
  if(alphaMatsOut) std::memcpy(alphaMatsOut, s->alphaMats.data(), sizeof(AlphaMat) * s->alphaMats.size());
  if(alphaMapsOut) std::memcpy(alphaMapsOut, s->alphaMaps.data(), 4 * s->alphaMaps.size());
  if(texelsOut) std::memcpy(texelsOut, s->texels.data(), 4 * s->texels.size());
}
// ALPHA_FAST_TAP cleared in every alpha record: opacity_eval then takes the general path (sample_rgba8_rec, wrap_index) and finds no map to ask
void th_clear_fast_tap(void* p)
{
  for(AlphaMat& a : static_cast<Scene*>(p)->alphaMats)
    a.texWrap &= ~ALPHA_FAST_TAP;
}

}  // extern "C"
