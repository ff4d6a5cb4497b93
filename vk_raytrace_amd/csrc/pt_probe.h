// Per-function probe of the shading source (test infrastructure, not part of include/pt_api.h): one state in, one result out, through the very
// functions shade_path calls -- bsdf_eval / bsdf_sample (disney_*, gltf_*), sun_and_sky, spherical_uv, make_frame, range / spot attenuation and the
// GLSL built-ins of pt_math.h (mirror, bend, lerp, smooth).  No formula lives here.  pt_debug.hip wraps it in a kernel (k_shading_probe, one state
// per lane); tests/cpp/trace_host.cpp compiles the same function for the host (th_shading_probe).  tests/test_float_kat.py holds both to an
// independent float64 model and to each other, bit for bit.  Below it: texture_probe (the software texture path one call at a time, tests/test_texture_model.py)
// and surface_probe (a hit turned into the Surface: fetch_triangle, surface_at_hit, resolve_material_at, and the per-slot shading lines; tests/test_surface_model.py),
// and trace_probe (the intersection arithmetic of pt_trace.h one call at a time: tri_test, world_tri, make_raybox, a node visit in both node forms, cn_plane,
// enter_instance; tests/test_trace_model.py).
//
// Row layouts (32-bit words; integers travel as bit patterns):
//   PROBE_EVAL_DISNEY / PROBE_EVAL_GLTF      in  m[22] N[3] T[3] B[3] eta thin V[3] L[3] seed   (PROBE_BSDF_IN = 40; m = albedo3 specular anisotropy metallic roughness subsurface specularTint sheen sheenTint3 clearcoat clearcoatRoughness transmission ior ax ay f0_3)
//                                            out f[3] pdf
//   PROBE_SAMPLE_DISNEY / PROBE_SAMPLE_GLTF  in  the same row (L unused)                        out L[3] f[3] pdf seed
//   PROBE_SUN_AND_SKY                        in  pt_SunAndSky[24] dir[3]                        out rgb[3]
//   PROBE_SPHERICAL_UV                       in  dir[3]                                         out uv[2]
//   PROBE_FRAME                              in  N[3]                                           out T[3] B[3]
//   PROBE_RANGE_ATTENUATION                  in  range distance                                 out 1
//   PROBE_SPOT_ATTENUATION                   in  pointToLight[3] spotDir[3] outerCos innerCos   out 1
//   PROBE_MIRROR                             in  I[3] N[3]                                      out 3
//   PROBE_BEND                               in  I[3] N[3] eta                                  out 3
//   PROBE_LERP                               in  a[3] b[3] t                                    out 3
//   PROBE_SMOOTH                             in  e0 e1 x                                        out 1
//   PROBE_ENV_SAMPLE                         in  xi[3] width height pad[3] pt_EnvAccel[width * height <= 8]   out toLight[3] pdf   (env_importance_sample; the radiance it returns is the sampler's business)
//   PROBE_CROSS                              in  a[3] b[3]                                      out 3   (cross3)
//   PROBE_UNIT                               in  a[3]                                           out 3   (unit = GLSL normalize)
//   PROBE_MAT4_VEC4                          in  m[16] column-major, v[4]                       out 4   (mat4_mul = mat4 * vec4)
//   PROBE_VEC4_MAT4                          no such function in the product (number kept in step with oracle/probe_rows.h)
//   PROBE_XFORM_POINT / _ROWVEC / _DIR       in  m[12] = 4 columns of vec3 (a GLSL mat4x3), p[3] out 3   (M * vec4(p, 1), vec3(p * M), mat4(M) * vec4(p, 0) on the Affine rows)
//   PROBE_BASIS_MUL                          in  c0[3] c1[3] c2[3] v[3]                         out 3   (mat3(c0, c1, c2) * v)
#pragma once
#include "pt_shade.h"
#include "pt_cnode.h"

enum {
  PROBE_EVAL_DISNEY = 0, PROBE_EVAL_GLTF, PROBE_SAMPLE_DISNEY, PROBE_SAMPLE_GLTF, PROBE_SUN_AND_SKY, PROBE_SPHERICAL_UV, PROBE_FRAME, PROBE_RANGE_ATTENUATION,
  PROBE_SPOT_ATTENUATION, PROBE_MIRROR, PROBE_BEND, PROBE_LERP, PROBE_SMOOTH, PROBE_ENV_SAMPLE, PROBE_CROSS, PROBE_UNIT, PROBE_MAT4_VEC4, PROBE_VEC4_MAT4,
  PROBE_XFORM_POINT, PROBE_XFORM_ROWVEC, PROBE_XFORM_DIR, PROBE_BASIS_MUL, PROBE_COUNT
};
enum { PROBE_BSDF_IN = 40, PROBE_ENV_TEXELS = 8, PROBE_SKY_WORDS = int(sizeof(pt_SunAndSky) / 4) };

// words a row of function fn must hold (0: no such function)
__host__ __device__ inline void probe_row_words(int fn, int& in, int& out)
{
  switch(fn)
  {
    case PROBE_EVAL_DISNEY: case PROBE_EVAL_GLTF: in = PROBE_BSDF_IN; out = 4; break;
    case PROBE_SAMPLE_DISNEY: case PROBE_SAMPLE_GLTF: in = PROBE_BSDF_IN; out = 8; break;
    case PROBE_SUN_AND_SKY: in = PROBE_SKY_WORDS + 3; out = 3; break;
    case PROBE_SPHERICAL_UV: in = 3; out = 2; break;
    case PROBE_FRAME: in = 3; out = 6; break;
    case PROBE_RANGE_ATTENUATION: in = 2; out = 1; break;
    case PROBE_SPOT_ATTENUATION: in = 8; out = 1; break;
    case PROBE_MIRROR: in = 6; out = 3; break;
    case PROBE_BEND: case PROBE_LERP: in = 7; out = 3; break;
    case PROBE_SMOOTH: in = 3; out = 1; break;
    case PROBE_ENV_SAMPLE: in = 8 + 4 * PROBE_ENV_TEXELS; out = 4; break;
    case PROBE_CROSS: in = 6; out = 3; break;
    case PROBE_UNIT: in = 3; out = 3; break;
    case PROBE_MAT4_VEC4: in = 20; out = 4; break;
    case PROBE_XFORM_POINT: case PROBE_XFORM_ROWVEC: case PROBE_XFORM_DIR: in = 15; out = 3; break;
    case PROBE_BASIS_MUL: in = 12; out = 3; break;
    default: in = 0; out = 0; break;
  }
}

PT_DEV f3 probe_f3(const float* p) { return f3{p[0], p[1], p[2]}; }
PT_DEV void probe_put(float* o, f3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }

PT_DEV void probe_surface(Surface& s, const float* r)
{
  const float* m = r;
  s.position = splat3(0.0f); s.normal = probe_f3(r + 22); s.ffnormal = s.normal; s.tangent = probe_f3(r + 25); s.bitangent = probe_f3(r + 28); s.uv = f2{0.0f, 0.0f};
  s.albedo = probe_f3(m); s.specular = m[3]; s.emission = splat3(0.0f); s.anisotropy = m[4]; s.metallic = m[5]; s.roughness = m[6];
  s.subsurface = m[7]; s.specularTint = m[8]; s.sheen = m[9]; s.sheenTint = probe_f3(m + 10); s.clearcoat = m[13];
  s.clearcoatRoughness = m[14]; s.transmission = m[15]; s.ior = m[16]; s.attenuationColor = splat3(1.0f); s.attenuationDistance = 1.0f;
  s.ax = m[17]; s.ay = m[18]; s.f0 = probe_f3(m + 19); s.alpha = 1.0f; s.unlit = false;
  s.eta = r[31]; s.thinwalled = r[32] != 0.0f;
}

PT_DEV void shading_probe(int fn, const float* in, float* out)
{
  switch(fn)
  {
    case PROBE_EVAL_DISNEY:
    case PROBE_EVAL_GLTF:
    {
      Surface s;
      probe_surface(s, in);
      float pdf = 0.0f;
      probe_put(out, bsdf_eval(fn - PROBE_EVAL_DISNEY, s, probe_f3(in + 33), s.ffnormal, probe_f3(in + 36), pdf));
      out[3] = pdf;
      break;
    }
    case PROBE_SAMPLE_DISNEY:
    case PROBE_SAMPLE_GLTF:
    {
      Surface s;
      probe_surface(s, in);
      float    pdf  = 0.0f;
      uint32_t seed = __float_as_uint(in[39]);
      f3       L    = splat3(0.0f);
      const f3 f    = bsdf_sample(fn - PROBE_SAMPLE_DISNEY, s, probe_f3(in + 33), s.ffnormal, L, pdf, seed);
      probe_put(out, L);
      probe_put(out + 3, f);
      out[6] = pdf;
      out[7] = __uint_as_float(seed);
      break;
    }
    case PROBE_SUN_AND_SKY:
    {
      pt_SunAndSky ss;
      float        w[PROBE_SKY_WORDS];
      for(int k = 0; k < PROBE_SKY_WORDS; ++k)
        w[k] = in[k];
      memcpy(&ss, w, sizeof(ss));
      probe_put(out, sun_and_sky(ss, probe_f3(in + PROBE_SKY_WORDS)));
      break;
    }
    case PROBE_SPHERICAL_UV:
    {
      const f2 uv = spherical_uv(probe_f3(in));
      out[0] = uv.x; out[1] = uv.y;
      break;
    }
    case PROBE_FRAME:
    {
      f3 T, B;
      make_frame(probe_f3(in), T, B);
      probe_put(out, T);
      probe_put(out + 3, B);
      break;
    }
    case PROBE_RANGE_ATTENUATION: out[0] = range_attenuation(in[0], in[1]); break;
    case PROBE_SPOT_ATTENUATION: out[0] = spot_attenuation(probe_f3(in), probe_f3(in + 3), in[6], in[7]); break;
    case PROBE_MIRROR: probe_put(out, mirror(probe_f3(in), probe_f3(in + 3))); break;
    case PROBE_BEND: probe_put(out, bend(probe_f3(in), probe_f3(in + 3), in[6])); break;
    case PROBE_LERP: probe_put(out, lerp(probe_f3(in), probe_f3(in + 3), in[6])); break;
    case PROBE_SMOOTH: out[0] = smooth(in[0], in[1], in[2]); break;
    case PROBE_ENV_SAMPLE:
    {
      const int w = int(in[3]), h = int(in[4]);
      if(w < 1 || h < 1 || w * h > PROBE_ENV_TEXELS)
        break;
      pt_EnvAccel acc[PROBE_ENV_TEXELS];
      float4      texels[PROBE_ENV_TEXELS];
      for(int k = 0; k < PROBE_ENV_TEXELS; ++k)
      {
        acc[k].alias = __float_as_uint(in[8 + 4 * k]); acc[k].q = in[9 + 4 * k]; acc[k].pdf = in[10 + 4 * k]; acc[k].aliasPdf = in[11 + 4 * k];
        texels[k] = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
      }
      DeviceScene S;
      memset(&S, 0, sizeof(S));
      S.env = texels; S.envAccel = acc; S.envW = w; S.envH = h;
      f3    toLight = splat3(0.0f);
      float pdf     = 0.0f;
      (void)env_importance_sample(S, probe_f3(in), toLight, pdf);
      probe_put(out, toLight);
      out[3] = pdf;
      break;
    }
    case PROBE_CROSS: probe_put(out, cross3(probe_f3(in), probe_f3(in + 3))); break;
    case PROBE_UNIT: probe_put(out, unit(probe_f3(in))); break;
    case PROBE_MAT4_VEC4:
    {
      const f4 r = mat4_mul(in, f4{in[16], in[17], in[18], in[19]});
      out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
      break;
    }
    case PROBE_XFORM_POINT:
    case PROBE_XFORM_ROWVEC:
    case PROBE_XFORM_DIR:
    {
      Affine m;  // row r of the column-major matrix, as the scene records store it
      m.r0 = make_float4(in[0], in[3], in[6], in[9]); m.r1 = make_float4(in[1], in[4], in[7], in[10]); m.r2 = make_float4(in[2], in[5], in[8], in[11]);
      const f3 p = probe_f3(in + 12);
      probe_put(out, fn == PROBE_XFORM_POINT ? xform_point(m, p) : fn == PROBE_XFORM_ROWVEC ? xform_rowvec(p, m) : xform_dir(m, p));
      break;
    }
    case PROBE_BASIS_MUL: probe_put(out, basis_mul(probe_f3(in), probe_f3(in + 3), probe_f3(in + 6), probe_f3(in + 9))); break;
    default: break;
  }
}

// ---- the software texture path one call at a time (tests/test_texture_model.py): the functions of pt_surface.h / pt_device.h on the records and the pool of
// a scene that is loaded -- tex_tap / tex_filter as resolve_material uses them, sample_rgba8_rec, opacity_eval with and without the opacity map, sample_env,
// wrap_index, tex_index.  No formula lives here either.  Rows of TEXP_IN words in, TEXP_OUT words out (integers travel as bit patterns):
//   TEXP_TAP          in  id slot u v       out i[4] a b     slot -1: the plain record texRecs[id]; 0..3: that descriptor of material id's line.  NO loads.
//   TEXP_SAMPLE_REC   in  id - u v          out rgba         sample_rgba8_rec on texRecs[id]
//   TEXP_SAMPLE_DESC  in  material slot u v out rgba         tex_desc_unpack, tex_tap, four loads, tex_filter: the lines of resolve_material
//   TEXP_OPACITY      in  uv0[2] uv1[2] uv2[2] material bu bv   out opacity_eval<false>, opacity_eval<true>
//   TEXP_ENV          in  u v               out rgb          sample_env
//   TEXP_WRAP         in  i n mode pot      out wrap_index
//   TEXP_INDEX        in  w ix iy tiled     out tex_index
//   TEXP_DESC         in  id slot           out offset w h mag wrapS wrapT pot tiled of tex_desc_unpack(tex_desc_pack(r)), r the record TEXP_TAP would use
// The kinds that load leave a row alone (its output stays as the caller filled it) unless every texel index of its tap is below `poolTexels` and its
// coordinates are inside the domain of the numerical contract (|u W|, |v H| < 2^30): a probe must not be able to read outside the pool.
enum { TEXP_TAP = 0, TEXP_SAMPLE_REC, TEXP_SAMPLE_DESC, TEXP_OPACITY, TEXP_ENV, TEXP_WRAP, TEXP_INDEX, TEXP_DESC, TEXP_COUNT };
enum { TEXP_IN = 12, TEXP_OUT = 8 };
struct TexProbeLimits {
  uint32_t numTexRecs, numMaterials, poolTexels;  // what the scene's arrays hold
};

PT_DEV bool texp_in_domain(const TexRec& tr, f2 uv) { return fabsf(uv.x * float(tr.w)) < 1073741824.0f && fabsf(uv.y * float(tr.h)) < 1073741824.0f; }
PT_DEV bool texp_record(const DeviceScene& S, const TexProbeLimits& lim, int id, int slot, TexRec& tr)
{
  if(id < 0 || slot < -1 || slot > 3)
    return false;
  if(slot < 0)
  {
    if(uint32_t(id) >= lim.numTexRecs)
      return false;
    tr = S.texRecs[id];
    return true;
  }
  if(uint32_t(id) >= lim.numMaterials)
    return false;
  tr = tex_desc_unpack(S.matLines[size_t(id) * PT_MAT_LINE_QUADS + 3 + slot]);
  return true;
}

PT_DEV void texture_probe(const DeviceScene& S, const TexProbeLimits& lim, int kind, const float* in, float* out)
{
  const int i0 = __float_as_int(in[0]), i1 = __float_as_int(in[1]);
  const f2  uv = f2{in[2], in[3]};
  switch(kind)
  {
    case TEXP_TAP:
    case TEXP_SAMPLE_REC:
    case TEXP_SAMPLE_DESC:
    {
      TexRec tr;
      if(!texp_record(S, lim, i0, kind == TEXP_SAMPLE_REC ? -1 : i1, tr))
        break;
      const TexTap t = tex_tap(tr, uv);
      if(kind == TEXP_TAP)
      {
        for(int k = 0; k < 4; ++k)
          out[k] = __uint_as_float(t.i[k]);
        out[4] = t.a; out[5] = t.b;
        break;
      }
      if(!texp_in_domain(tr, uv) || t.i[0] >= lim.poolTexels || t.i[1] >= lim.poolTexels || t.i[2] >= lim.poolTexels || t.i[3] >= lim.poolTexels)
        break;
      const f4 c = kind == TEXP_SAMPLE_REC ? sample_rgba8_rec(S.texels, tr, uv) : tex_filter(t, S.texels[t.i[0]], S.texels[t.i[1]], S.texels[t.i[2]], S.texels[t.i[3]]);
      out[0] = c.x; out[1] = c.y; out[2] = c.z; out[3] = c.w;
      break;
    }
    case TEXP_OPACITY:
    {
      const uint32_t m = __float_as_uint(in[6]);
      if(m >= lim.numMaterials)
        break;
      bool ok = true;  // |coordinates| <= 4 and |uvTransform| <= 16 keep the transformed coordinate far inside the domain for every image size
      for(int k = 0; k < 9; ++k)
        ok = ok && (k == 6 || fabsf(in[k]) <= 4.0f);
      for(int k = 0; k < 8; ++k)
        ok = ok && fabsf(S.alphaMats[m].m[k]) <= 16.0f;
      if(!ok)
        break;
      AlphaRec ar;
      ar.uv0[0] = in[0]; ar.uv0[1] = in[1]; ar.uv1[0] = in[2]; ar.uv1[1] = in[3]; ar.uv2[0] = in[4]; ar.uv2[1] = in[5];
      ar.material = m; ar._pad = 0u;
      out[0] = opacity_eval<false>(S, ar, in[7], in[8]);
      out[1] = opacity_eval<true>(S, ar, in[7], in[8]);
      break;
    }
    case TEXP_ENV:
    {
      const f2 e = f2{in[0], in[1]};
      if(S.env == nullptr || S.envW < 1 || S.envH < 1 || !(fabsf(e.x * float(S.envW)) < 1073741824.0f && fabsf(e.y * float(S.envH)) < 1073741824.0f))
        break;
      probe_put(out, sample_env(S, e));
      break;
    }
    case TEXP_WRAP: out[0] = __int_as_float(wrap_index(i0, i1, __float_as_int(in[2]), __float_as_int(in[3]) != 0)); break;
    case TEXP_INDEX: out[0] = __uint_as_float(tex_index(i0, i1, __float_as_int(in[2]), __float_as_int(in[3]) != 0)); break;
    case TEXP_DESC:
    {
      TexRec tr;
      if(!texp_record(S, lim, i0, i1, tr))
        break;
      const TexRec   r    = tex_desc_unpack(tex_desc_pack(tr));
      const uint32_t w[8] = {r.offset, uint32_t(r.w), uint32_t(r.h), uint32_t(r.mag), uint32_t(r.wrapS), uint32_t(r.wrapT), uint32_t(r.pot), uint32_t(r.tiled)};
      for(int k = 0; k < 8; ++k)
        out[k] = __uint_as_float(w[k]);
      break;
    }
    default: break;
  }
}

// ---- a hit turned into the Surface every BSDF call reads (tests/test_surface_model.py): fetch_triangle, surface_at_hit, the ffnormal line, resolve_material_at
// and the vertex-colour line, on the instances / vertices / materials / pool of a scene that is loaded.  No formula lives here; pt_shade.h is left alone
// (factoring its lines 257-267 into a function of their own is not worth a different pt_render.o), so the three glue lines between the calls are REPEATED
// below, word for word.  Rows of SURF_IN words in, SURF_OUT words out (integers travel as bit patterns):
//   SURF_STATE  in  instance primitive bu bv rayDir[3] path     path 0: what shade_path does (resolve_material_at); 1: the full material record, always
//               out after surface_at_hit  position[3] normal[3] tangent[3] bitangent[3] uv[2] vcolor[3]                                  (words 0-16)
//                   after the resolve     position[3] normal[3] ffnormal[3] tangent[3] bitangent[3] uv[2] albedo[3] (x vcolor) emission[3] f0[3] metallic
//                                         roughness ax ay anisotropy clearcoat clearcoatRoughness transmission ior eta attenuationColor[3]
//                                         attenuationDistance alpha sheen sheenTint[3] specular specularTint subsurface unlit thinwalled   (words 17-66)
//                   material index used, 1 when the material came from its 128-byte line alone (MAT_SIMPLE)                              (words 67-68)
//   SURF_SLOT   in  slot                                        out the six float4 of the slot's shading line (words 0-23), then instance primitive material 0
//               surface_probe returns SURF_NO_DATA (and touches nothing) when the scene has no shading lines
// A row is left alone (its output stays as the caller filled it) unless its instance, primitive, vertex indices, material, slot and every texture the material
// names lie inside what the scene's arrays hold: a probe must not be able to read outside them.  A texture is inside when its whole image is (every tap of
// tex_tap / sample_rgba8_rec lands in the image for every float coordinate, texel_coord), so no coordinate has to be known before the resolve runs.
enum { SURF_STATE = 0, SURF_SLOT, SURF_COUNT };
enum { SURF_IN = 8, SURF_OUT = 72, SURF_FRAME_WORDS = 17, SURF_WORDS = 69, SURF_OK = 0, SURF_NO_DATA = 1 };
struct SurfProbeLimits {
  uint32_t numInstances, numIndices, numVertices, numMaterials, numTexRecs, poolTexels, numSlots;  // what the scene's arrays hold
};

PT_DEV bool surfp_texture_inside(const TexRec& tr, const SurfProbeLimits& lim)
{
  if(tr.w < 1 || tr.h < 1 || tr.w > 65535 || tr.h > 65535)
    return false;
  return uint64_t(tr.offset) + uint64_t(tr.w) * uint64_t(tr.h) * tex_layers(tr) <= uint64_t(lim.poolTexels);
}
PT_DEV bool surfp_material_inside(const DeviceScene& S, const SurfProbeLimits& lim, int m)
{
  if(m < 0 || uint32_t(m) >= lim.numMaterials)
    return false;
  const uint4*   line  = S.matLines + size_t(m) * PT_MAT_LINE_QUADS;
  const uint32_t flags = line[2].w;
  const uint32_t has[4] = {MAT_HAS_NORMAL, MAT_HAS_EMISSIVE, MAT_HAS_MR, MAT_HAS_BASE};
  const pt_GltfShadeMaterial& r = S.materials[m];
  const int      ids[4] = {r.normalTexture, r.emissiveTexture, r.pbrMetallicRoughnessTexture, r.pbrBaseColorTexture};
  for(int k = 0; k < 4; ++k)
  {
    if(((flags & has[k]) != 0) != (ids[k] > -1))  // line and record name the same textures
      return false;
    if((flags & has[k]) && !surfp_texture_inside(tex_desc_unpack(line[3 + k]), lim))
      return false;
  }
  const int more[3] = {r.transmissionTexture, r.clearcoatTexture, r.clearcoatRoughnessTexture};
  for(int k = 0; k < 3; ++k)
    if(more[k] > -1 && (uint32_t(more[k]) >= lim.numTexRecs || !surfp_texture_inside(S.texRecs[more[k]], lim)))
      return false;
  return true;
}
PT_DEV void surfp_put2(float* o, f2 v) { o[0] = v.x; o[1] = v.y; }

PT_DEV int surface_probe(const DeviceScene& S, const SurfProbeLimits& lim, int kind, const float* in, float* out)
{
  if(kind == SURF_SLOT)
  {
    if(S.shadeTris == nullptr)
      return SURF_NO_DATA;
    const uint32_t slot = __float_as_uint(in[0]);
    if(slot >= lim.numSlots)
      return SURF_OK;
    const VertexTriple v = fetch_triangle_slot(S, slot);
    const float4       q[7] = {v.a0, v.b0, v.a1, v.b1, v.a2, v.b2, S.shadeTris[size_t(slot) * PT_SHADE_REC_QUADS + 6]};
    for(int k = 0; k < 7; ++k)
    {
      out[4 * k] = q[k].x; out[4 * k + 1] = q[k].y; out[4 * k + 2] = q[k].z; out[4 * k + 3] = q[k].w;
    }
    return SURF_OK;
  }
  if(kind != SURF_STATE)
    return SURF_OK;
  const uint32_t hitInst = __float_as_uint(in[0]), hitPrim = __float_as_uint(in[1]), path = __float_as_uint(in[7]);
  if(hitInst >= lim.numInstances || path > 1u)
    return SURF_OK;
  const InstanceRec& I = S.instances[hitInst];
  if(hitPrim >= I.triCount || uint64_t(I.firstIndex) + 3ull * hitPrim + 3ull > uint64_t(lim.numIndices))
    return SURF_OK;
  for(int k = 0; k < 3; ++k)
    if(uint64_t(I.vertexOffset) + uint64_t(S.indices[I.firstIndex + 3 * size_t(hitPrim) + k]) >= uint64_t(lim.numVertices))
      return SURF_OK;
  const int matIndex = I.materialIndex;
  const int useMat   = matIndex < 0 ? 0 : matIndex;
  if(!surfp_material_inside(S, lim, useMat))
    return SURF_OK;
  const f3 rdir = probe_f3(in + 4);

  Surface            sf;
  f3                 vcolor;
  const VertexTriple vt = fetch_triangle(S, I, hitPrim);
  surface_at_hit(S, I, vt, in[2], in[3], sf, vcolor);
  probe_put(out, sf.position); probe_put(out + 3, sf.normal); probe_put(out + 6, sf.tangent); probe_put(out + 9, sf.bitangent);
  surfp_put2(out + 12, sf.uv); probe_put(out + 14, vcolor);
  // pt_shade.h:264-267, repeated
  sf.ffnormal = dot3(sf.normal, rdir) <= 0.0f ? sf.normal : -sf.normal;
  bool line   = false;
  if(path == 0u)
  {
    line = (S.matLines[size_t(useMat) * PT_MAT_LINE_QUADS + 2].w & MAT_SIMPLE) != 0;
    resolve_material_at(S, matIndex < 0 ? 0 : matIndex, rdir, sf);
  }
  else
  {
    const uint4* l     = S.matLines + size_t(useMat) * PT_MAT_LINE_QUADS;
    const uint4  md[4] = {l[3], l[4], l[5], l[6]};
    resolve_material(S, S.materials[useMat], md, rdir, sf);
  }
  sf.albedo *= vcolor;

  float* o = out + SURF_FRAME_WORDS;
  probe_put(o, sf.position); probe_put(o + 3, sf.normal); probe_put(o + 6, sf.ffnormal); probe_put(o + 9, sf.tangent); probe_put(o + 12, sf.bitangent);
  surfp_put2(o + 15, sf.uv); probe_put(o + 17, sf.albedo); probe_put(o + 20, sf.emission); probe_put(o + 23, sf.f0);
  o[26] = sf.metallic; o[27] = sf.roughness; o[28] = sf.ax; o[29] = sf.ay; o[30] = sf.anisotropy; o[31] = sf.clearcoat; o[32] = sf.clearcoatRoughness;
  o[33] = sf.transmission; o[34] = sf.ior; o[35] = sf.eta; probe_put(o + 36, sf.attenuationColor); o[39] = sf.attenuationDistance; o[40] = sf.alpha;
  o[41] = sf.sheen; probe_put(o + 42, sf.sheenTint); o[45] = sf.specular; o[46] = sf.specularTint; o[47] = sf.subsurface;
  o[48] = __uint_as_float(sf.unlit ? 1u : 0u); o[49] = __uint_as_float(sf.thinwalled ? 1u : 0u);
  o[50] = __uint_as_float(uint32_t(useMat)); o[51] = __uint_as_float(line ? 1u : 0u);
  return SURF_OK;
}

// ---- the intersection arithmetic one call at a time (tests/test_trace_model.py, tests/test_trace_gpu.py): tri_test (trace contract T2 / T3), world_tri (T1 at a
// two-level leaf), make_raybox, one node visit on the 128-byte node (wide_node_step) and on its 80-byte form (cn_encode, then wide_node_step_c), cn_plane and
// enter_instance.  No formula lives here.  Every load stays inside the row: the node, the instance record and the TLAS leaf a function reads are built from the
// row's words on the stack.  Rows of up to TRP_IN words in, TRP_OUT words out (integers travel as bit patterns; trace_row_words has the counts per kind):
//   TRP_TRI        in  p0[3] e1[3] e2[3] flags o[3] d[3]              out accept, t u v (left as the caller filled them on reject)
//   TRP_WORLD_TRI  in  objectToWorld r0[4] r1[4] r2[4], v0[3] v1[3] v2[3] (object space)   out p0[3] e1[3] e2[3] of world_tri
//   TRP_RAYBOX     in  o[3] d[3]                                      out idir[3] nlo[3] nhi[3] nearOff[3]
//   TRP_NODE       in  one WideNode: minx[4] miny[4] minz[4] maxx[4] maxy[4] maxz[4] child[4], then o[3] d[3] lim alphaOnly
//                  out the child returned, the number pushed, the pushed children in push order (the rest left alone)
//   TRP_CNODE      in  the same row                                   out cn_encode's ok flag, then the same five words from the visit of the encoded node
//                                                                         (left alone when the node cannot be encoded)
//   TRP_CN_PLANE   in  one word                                       out cn_plane(word, 0), cn_plane(word, 1)
//   TRP_ENTER      in  worldToObject r0[4] r1[4] r2[4], padC0 padC1, o[3] d[3]             out the RayBox of enter_instance, as TRP_RAYBOX
enum { TRP_TRI = 0, TRP_WORLD_TRI, TRP_RAYBOX, TRP_NODE, TRP_CNODE, TRP_CN_PLANE, TRP_ENTER, TRP_COUNT };
enum { TRP_IN = 36, TRP_OUT = 12 };

__host__ __device__ inline void trace_row_words(int kind, int& in, int& out)
{
  switch(kind)
  {
    case TRP_TRI: in = 16; out = 4; break;
    case TRP_WORLD_TRI: in = 21; out = 9; break;
    case TRP_RAYBOX: in = 6; out = 12; break;
    case TRP_NODE: in = 36; out = 5; break;
    case TRP_CNODE: in = 36; out = 6; break;
    case TRP_CN_PLANE: in = 1; out = 2; break;
    case TRP_ENTER: in = 20; out = 12; break;
    default: in = 0; out = 0; break;
  }
}

PT_DEV void trp_put_raybox(float* out, const RayBox& rb)
{
  probe_put(out, rb.idir); probe_put(out + 3, rb.nlo); probe_put(out + 6, rb.nhi);
  for(int a = 0; a < 3; ++a)
    out[9 + a] = __uint_as_float(rb.nearOff[a]);
}
PT_DEV Affine trp_affine(const float* r)
{
  Affine m;
  m.r0 = make_float4(r[0], r[1], r[2], r[3]); m.r1 = make_float4(r[4], r[5], r[6], r[7]); m.r2 = make_float4(r[8], r[9], r[10], r[11]);
  return m;
}

PT_DEV void trace_probe(int kind, const float* in, float* out)
{
  switch(kind)
  {
    case TRP_TRI:
    {
      TriRec tr;
      tr.p0w = make_float4(in[0], in[1], in[2], 0.0f); tr.e1n = make_float4(in[3], in[4], in[5], 0.0f); tr.e2p = make_float4(in[6], in[7], in[8], 0.0f);
      float      t = out[1], u = out[2], v = out[3];
      const bool hit = tri_test(tr, __float_as_uint(in[9]), probe_f3(in + 10), probe_f3(in + 13), t, u, v);
      out[0] = __uint_as_float(hit ? 1u : 0u);
      if(hit)
      {
        out[1] = t; out[2] = u; out[3] = v;
      }
      break;
    }
    case TRP_WORLD_TRI:
    {
      InstanceRec I;
      memset(&I, 0, sizeof(I));
      I.objectToWorld = trp_affine(in);
      DeviceScene S;
      memset(&S, 0, sizeof(S));
      S.instances = &I; S.numInstances = 1;
      TriRec obj;
      obj.p0w = make_float4(in[12], in[13], in[14], __uint_as_float(0u)); obj.e1n = make_float4(in[15], in[16], in[17], 0.0f); obj.e2p = make_float4(in[18], in[19], in[20], 0.0f);
      const TriRec r = world_tri(S, InstCtx{0u, 0, 0u}, obj);
      probe_put(out, xyz(r.p0w)); probe_put(out + 3, xyz(r.e1n)); probe_put(out + 6, xyz(r.e2p));
      break;
    }
    case TRP_RAYBOX: trp_put_raybox(out, make_raybox(probe_f3(in), probe_f3(in + 3))); break;
    case TRP_NODE:
    case TRP_CNODE:
    {
      WideNode w;
      memset(&w, 0, sizeof(w));
      float    planes[24];
      uint32_t cw[4];
      for(int k = 0; k < 24; ++k)
        planes[k] = in[k];
      for(int k = 0; k < 4; ++k)
        cw[k] = __float_as_uint(in[24 + k]);
      memcpy(&w, planes, sizeof(planes));  // minx .. maxz are the first 96 bytes of the node, in this order
      w.child[0] = make_uint4(cw[0], cw[1], cw[2], cw[3]);
      const RayBox rb        = make_raybox(probe_f3(in + 28), probe_f3(in + 31));
      const float  lim       = in[34];
      const bool   alphaOnly = __float_as_uint(in[35]) != 0u;
      uint32_t     pushed[PT_BVH_WIDTH];
      int          np   = 0;
      auto         push = [&](uint32_t c) {
        if(np < PT_BVH_WIDTH)
          pushed[np++] = c;
      };
      uint32_t nearest;
      float*   o = out;
      if(kind == TRP_CNODE)
      {
        CompactNode c;
        const bool  ok = cn_encode(w, c);
        out[0]         = __uint_as_float(ok ? 1u : 0u);
        if(!ok)
          break;
        nearest = wide_node_step_c(&c, 0u, rb, lim, alphaOnly, push);
        o       = out + 1;
      }
      else
        nearest = wide_node_step(&w, 0u, rb, lim, alphaOnly, push);
      o[0] = __uint_as_float(nearest);
      o[1] = __uint_as_float(uint32_t(np));
      for(int k = 0; k < np && k < 3; ++k)
        o[2 + k] = __uint_as_float(pushed[k]);
      break;
    }
    case TRP_CN_PLANE:
    {
      const uint32_t word = __float_as_uint(in[0]);
      out[0] = cn_plane(word, 0); out[1] = cn_plane(word, 1);
      break;
    }
    case TRP_ENTER:
    {
      InstanceRec I;
      memset(&I, 0, sizeof(I));
      I.worldToObject = trp_affine(in);
      DeviceScene S;
      memset(&S, 0, sizeof(S));
      S.instances = &I; S.numInstances = 1;
      TlasLeaf tl;
      memset(&tl, 0, sizeof(tl));
      tl.inst = 0u; tl.padC0 = in[12]; tl.padC1 = in[13];
      trp_put_raybox(out, enter_instance(S, tl, probe_f3(in + 14), probe_f3(in + 17)));
      break;
    }
    default: break;
  }
}
