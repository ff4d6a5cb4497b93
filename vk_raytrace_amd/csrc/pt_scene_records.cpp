// Pure host code of the library: what pt_set_scene derives from a scene description before anything is uploaded (build_scene_records), the
// per-instance transform records, the padding bound of the two-level walk, the tail-takeover decision and the PT_TUNE parser -- and the
// no-GPU test hooks built on them.  The CPU test suite treats this unit as the product's host model.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include "pt_internal.h"
#include "pt_scene_records.h"

// inverse of an affine column-major 4x4 (last row forced to 0 0 0 1), computed in double and rounded once
static bool affine_inverse(const float* m, double inv[12], double& det3)
{
  const double a = m[0], b = m[4], c = m[8], d = m[1], e = m[5], f = m[9], g = m[2], h = m[6], i = m[10];
  const double tx = m[12], ty = m[13], tz = m[14];
  const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
  det3 = a * A + b * B + c * C;
  if(det3 == 0.0)
    return false;
  const double r = 1.0 / det3;
  // rows of the inverse 3x3
  const double i00 = A * r, i01 = -(b * i - c * h) * r, i02 = (b * f - c * e) * r;
  const double i10 = B * r, i11 = (a * i - c * g) * r, i12 = -(a * f - c * d) * r;
  const double i20 = C * r, i21 = -(a * h - b * g) * r, i22 = (a * e - b * d) * r;
  // column-major 3x4: columns 0..2 then translation
  inv[0] = i00; inv[1] = i10; inv[2] = i20;
  inv[3] = i01; inv[4] = i11; inv[5] = i21;
  inv[6] = i02; inv[7] = i12; inv[8] = i22;
  inv[9]  = -(i00 * tx + i01 * ty + i02 * tz);
  inv[10] = -(i10 * tx + i11 * ty + i12 * tz);
  inv[11] = -(i20 * tx + i21 * ty + i22 * tz);
  return true;
}

// fills the per-instance part of an InstanceRec that depends on the node's world matrix (pt_set_scene, pt_update_instances)
bool set_instance_transform(InstanceRec& I, const float* m, uint32_t materialFlags)
{
  I.objectToWorld.r0 = make_float4(m[0], m[4], m[8], m[12]);
  I.objectToWorld.r1 = make_float4(m[1], m[5], m[9], m[13]);
  I.objectToWorld.r2 = make_float4(m[2], m[6], m[10], m[14]);
  double inv[12], det3;
  if(!affine_inverse(m, inv, det3))
    return false;
  I.worldToObject.r0 = make_float4(float(inv[0]), float(inv[3]), float(inv[6]), float(inv[9]));
  I.worldToObject.r1 = make_float4(float(inv[1]), float(inv[4]), float(inv[7]), float(inv[10]));
  I.worldToObject.r2 = make_float4(float(inv[2]), float(inv[5]), float(inv[8]), float(inv[11]));
  I.flags = (materialFlags & ~TRI_FLIP) | (det3 < 0.0 ? TRI_FLIP : 0u);
  return true;
}

// Two-level walk: how far the object-space image of a world-space hit point can lie from the transformed ray (TlasLeaf::padC0 / padC1,
// pt_trace.h enter_instance).  With u = 2^-24, A = max abs row sum of the 3x3 parts, T = max |translation|, Bo = max |object coordinate|
// of the mesh, |p| <= Am Bo + Tm for every world point of the instance:
//   ray transform          <= u (7 Ainv |o| + 3 Ainv |p| + 4 Tinv)          (4-term dot products for o', 3-term for d', scaled by t |d| <= |p| + |o|)
//   inverse rounded to f32 <= u (Ainv |p| + Tinv)
//   T1 rounding of the world triangle, seen from object space <= 4 u Ainv (Am Bo + Tm)
//   the triangle test accepts points a few ulps of |p| off the triangle (the flat structure pads its leaf boxes by 67 u |p| for that)
// eps = 2^-17 (Ainv |o|  +  Ainv (Am Bo + 2 Tm) + Tinv + Bo) = 128 u (...) covers their sum with room to spare and is still ~1e-3 of a
// world unit for a scene 50 units across.
void two_level_pad(const InstanceRec& I, float Bo, float& c0, float& c1)
{
  auto rs = [](const float4& r) { return double(std::fabs(r.x)) + std::fabs(r.y) + std::fabs(r.z); };
  const double Am   = std::max(rs(I.objectToWorld.r0), std::max(rs(I.objectToWorld.r1), rs(I.objectToWorld.r2)));
  const double Tm   = std::max(std::fabs(double(I.objectToWorld.r0.w)), std::max(std::fabs(double(I.objectToWorld.r1.w)), std::fabs(double(I.objectToWorld.r2.w))));
  const double Ainv = std::max(rs(I.worldToObject.r0), std::max(rs(I.worldToObject.r1), rs(I.worldToObject.r2)));
  const double Tinv = std::max(std::fabs(double(I.worldToObject.r0.w)), std::max(std::fabs(double(I.worldToObject.r1.w)), std::fabs(double(I.worldToObject.r2.w))));
  const double k    = 1.0 / 131072.0;  // 2^-17
  const double v1 = k * Ainv, v0 = k * (Ainv * (Am * double(Bo) + 2.0 * Tm) + Tinv + double(Bo));
  c1 = std::nextafter(float(std::min(v1, 1e30)), INFINITY);
  c0 = std::nextafter(float(std::min(v0, 1e30)), INFINITY);
}

// Opacity maps (pt_device.h): for every non-opaque material whose base-colour texture takes the fast tap, classify each
// ALPHA_MAP_BLOCK^2 block of base texels + one texel of apron on every side (a bilinear tap based in the block blends
// texels of that window only).  A state is assigned only when every texel of the window decides the same way with a
// 1e-5 relative margin -- two orders above the fp32 filtering error -- so the map never changes a result.
static void build_opacity_maps(const pt_SceneDesc* d, std::vector<AlphaMat>& am, std::vector<uint32_t>& words)
{
  struct Key {
    int   tex, mode;
    float factor, cutoff;
    bool  operator<(const Key& o) const { return std::tie(tex, mode, factor, cutoff) < std::tie(o.tex, o.mode, o.factor, o.cutoff); }
  };
  std::map<Key, uint32_t> done;
  words.assign(1, 0u);  // never empty (word 0 is unused padding)
  for(size_t m = 0; m < am.size(); ++m)
  {
    AlphaMat& a = am[m];
    if(a.mode == PT_ALPHA_OPAQUE || a.tex < 0 || !(a.texWrap & ALPHA_FAST_TAP) || a.texW < ALPHA_MAP_BLOCK || a.texH < ALPHA_MAP_BLOCK)
      continue;
    if(!(a.factorA >= 0.0f && a.factorA <= 3.0e38f) || !(std::fabs(a.cutoff) <= 3.0e38f))
      continue;
    const Key key{a.tex, a.mode, a.factorA, a.cutoff};
    auto      it = done.find(key);
    if(it != done.end())
    {
      a.mapOffset = it->second;
      continue;
    }
    const int      W = a.texW, H = a.texH, bw = W >> ALPHA_MAP_SHIFT, bh = H >> ALPHA_MAP_SHIFT;
    const uint8_t* px = (const uint8_t*)d->textures[a.tex].rgba8;
    // separable min / max of the alpha byte over [b*B - 1, b*B + B] (wrapped)
    std::vector<uint8_t> rmin(size_t(bw) * H), rmax(size_t(bw) * H);
    for(int y = 0; y < H; ++y)
      for(int bx = 0; bx < bw; ++bx)
      {
        uint8_t lo = 255, hi = 0;
        for(int k = -1; k <= ALPHA_MAP_BLOCK; ++k)
        {
          const uint8_t v = px[(size_t(y) * W + ((bx * ALPHA_MAP_BLOCK + k) & (W - 1))) * 4 + 3];
          lo = v < lo ? v : lo;
          hi = v > hi ? v : hi;
        }
        rmin[size_t(y) * bw + bx] = lo;
        rmax[size_t(y) * bw + bx] = hi;
      }
    const uint32_t off = uint32_t(words.size());
    words.resize(words.size() + (size_t(bw) * bh + 15) / 16, 0u);
    const double f = a.factorA, cut = a.cutoff;
    for(int by = 0; by < bh; ++by)
      for(int bx = 0; bx < bw; ++bx)
      {
        uint8_t lo = 255, hi = 0;
        for(int k = -1; k <= ALPHA_MAP_BLOCK; ++k)
        {
          const int y = (by * ALPHA_MAP_BLOCK + k) & (H - 1);
          lo = rmin[size_t(y) * bw + bx] < lo ? rmin[size_t(y) * bw + bx] : lo;
          hi = rmax[size_t(y) * bw + bx] > hi ? rmax[size_t(y) * bw + bx] : hi;
        }
        const double vmin = f * lo / 255.0, vmax = f * hi / 255.0;
        uint32_t     st = ALPHA_ST_UNKNOWN;
        if(a.mode == PT_ALPHA_MASK)
        {
          if(vmin > cut + 1e-5 * std::fmax(std::fabs(cut), vmin))
            st = ALPHA_ST_ONE;
          else if((hi == 0 && cut >= 0.0) || vmax < cut - 1e-5 * std::fmax(std::fabs(cut), vmax))
            st = ALPHA_ST_ZERO;
        }
        else  // BLEND: opacity = factor x filtered alpha
        {
          if(hi == 0 || f == 0.0)
            st = ALPHA_ST_ZERO;
          else if(vmin >= 1.0 + 1e-5)
            st = ALPHA_ST_ONE;
        }
        const uint32_t bidx = uint32_t(by) * uint32_t(bw) + uint32_t(bx);
        words[off + (bidx >> 4)] |= st << ((bidx & 15u) * 2u);
      }
    a.mapOffset = off;
    done[key]   = off;
  }
}

__attribute__((format(printf, 2, 3))) static int records_fail(std::string& err, const char* fmt, ...)
{
  char    buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  err = buf;
  return PT_ERR_INVALID;
}
void store_texture(uint32_t* dst, const TexRec& tr, const void* rgba8RowMajor)
{
  const uint32_t* src = static_cast<const uint32_t*>(rgba8RowMajor);
  if(!tr.tiled)
  {
    std::memcpy(dst, src, size_t(tr.w) * tr.h * 4);
    return;
  }
  for(int y = 0; y < tr.h; ++y)
    for(int x = 0; x < tr.w; x += PT_TEX_TILE_W)
      std::memcpy(dst + tex_index(tr.w, x, y, true), src + size_t(y) * tr.w + x, PT_TEX_TILE_W * 4);
}

void store_group(uint32_t* dst, const SceneRecords::TexGroup& g, const std::vector<TexRec>& texRecs, const pt_SceneDesc* d)
{
  for(int l = 0; l < g.layers; ++l)
  {
    const TexRec&   tr  = texRecs[size_t(g.tex[l])];
    const uint32_t* src = reinterpret_cast<const uint32_t*>(d->textures[g.tex[l]].rgba8);
    for(int y = 0; y < tr.h; ++y)
      for(int x = 0; x < tr.w; ++x)
        dst[size_t(tex_index(tr.w, x, y, (tr.tiled & 1) != 0)) * size_t(g.layers) + size_t(l)] = src[size_t(y) * tr.w + x];
  }
}

int build_scene_records(const pt_SceneDesc* d, SceneRecords& R, std::string& err, int texTile, int texGroups)
{
  if(!d || !d->vertices || !d->indices || !d->primMeshes || !d->nodes || !d->materials || d->numMaterials == 0)
    return records_fail(err, "pt_set_scene: null array or no material");
  if((d->numLights && !d->lights) || (d->numTextures && !d->textures))
    return records_fail(err, "pt_set_scene: count without array");
  // ---- validate + build the per-instance records
  R.inst.assign(d->numNodes, InstanceRec{});
  R.triTotal = 0;
  for(uint32_t n = 0; n < d->numNodes; ++n)
  {
    const pt_Node& nd = d->nodes[n];
    if(nd.primMesh < 0 || uint32_t(nd.primMesh) >= d->numPrimMeshes)
      return records_fail(err, "node %u: primMesh %d out of range", n, nd.primMesh);
    const pt_PrimMesh& pm = d->primMeshes[nd.primMesh];
    if(pm.materialIndex >= int(d->numMaterials))
      return records_fail(err, "primMesh %d: materialIndex %d out of range", nd.primMesh, pm.materialIndex);
    if(uint64_t(pm.vertexOffset) + pm.vertexCount > d->numVertices || uint64_t(pm.firstIndex) + pm.indexCount > d->numIndices || pm.indexCount % 3)
      return records_fail(err, "primMesh %d: vertex/index range out of bounds", nd.primMesh);
    const pt_GltfShadeMaterial& mat = d->materials[pm.materialIndex < 0 ? 0 : pm.materialIndex];
    InstanceRec&                I   = R.inst[n];
    // instance flags of the reference's TLAS (src/accelstruct.cpp:144-149)
    uint32_t flags = 0;
    if(mat.alphaMode == 0 || (mat.pbrBaseColorFactor[3] == 1.0f && mat.pbrBaseColorTexture == -1))
      flags |= TRI_OPAQUE;
    if(mat.doubleSided == 1)
      flags |= TRI_NOCULL;
    if(!set_instance_transform(I, nd.worldMatrix, flags))  // + TRI_FLIP for a mirroring matrix
      return records_fail(err, "node %u: singular world matrix", n);
    I.vertexOffset  = pm.vertexOffset;
    I.firstIndex    = pm.firstIndex;
    I.materialIndex = pm.materialIndex;
    I.primMesh      = nd.primMesh;
    I.triBase       = uint32_t(R.triTotal);
    I.triCount      = pm.indexCount / 3;
    I._pad  = 0;
    R.triTotal += I.triCount;
  }
  if(R.triTotal > TRI_INDEX_MASK)
    return records_fail(err, "scene has %llu triangles; the limit is %u", (unsigned long long)R.triTotal, TRI_INDEX_MASK);
  R.primBound.assign(d->numPrimMeshes, 0.f);
  for(uint32_t p = 0; p < d->numPrimMeshes; ++p)
  {
    const pt_PrimMesh& pm = d->primMeshes[p];
    for(uint32_t k = 0; k < pm.indexCount; ++k)
      if(d->indices[pm.firstIndex + k] >= pm.vertexCount)
        return records_fail(err, "primMesh %u: index %u >= vertexCount", p, d->indices[pm.firstIndex + k]);
    float b = 0.f;
    for(uint32_t v = 0; v < pm.vertexCount; ++v)
    {
      const float* q = d->vertices[pm.vertexOffset + v].position;
      for(int a = 0; a < 3; ++a)
        if(std::isfinite(q[a]))
          b = std::max(b, std::fabs(q[a]));
    }
    R.primBound[p] = b;
  }
  for(uint32_t m = 0; m < d->numMaterials; ++m)
  {
    const pt_GltfShadeMaterial& mt = d->materials[m];
    const int ids[] = {mt.pbrBaseColorTexture, mt.pbrMetallicRoughnessTexture, mt.emissiveTexture, mt.normalTexture, mt.transmissionTexture, mt.clearcoatTexture, mt.clearcoatRoughnessTexture};
    for(int id : ids)
      if(id >= int(d->numTextures))
        return records_fail(err, "material %u references texture %d of %u", m, id, d->numTextures);
  }
  // ---- texture records (one RGBA8 pool)
  R.texRecs.assign(d->numTextures ? d->numTextures : 1, TexRec{});
  R.texels = 0;
  for(uint32_t t = 0; t < d->numTextures; ++t)
  {
    const pt_TextureDesc& td = d->textures[t];
    if(!td.rgba8 || td.width <= 0 || td.height <= 0)
      return records_fail(err, "texture %u: empty image", t);
    if(td.width > 65535 || td.height > 65535)  // (pt_device.h tex_index multiplies row x stride in 24 bits)
      return records_fail(err, "texture %u: %d x %d exceeds 65535 texels a side (tex_desc_pack keeps a side in 16 bits)", t, td.width, td.height);
    R.texRecs[t].tiled  = (texTile && td.width % PT_TEX_TILE_W == 0 && td.height % PT_TEX_TILE_H == 0) ? 1 : 0;
    if(R.texRecs[t].tiled)
      R.texels = (R.texels + 31u) & ~size_t(31);  // a tile = one 128-byte line (the pool itself is 256-byte aligned)
    R.texRecs[t].offset = uint32_t(R.texels);
    R.texRecs[t].w      = td.width;
    R.texRecs[t].h      = td.height;
    R.texRecs[t].mag    = td.magFilter;
    R.texRecs[t].wrapS  = td.wrapS;
    R.texRecs[t].wrapT  = td.wrapT;
    R.texRecs[t].pot    = ((td.width & (td.width - 1)) == 0 ? 1 : 0) | ((td.height & (td.height - 1)) == 0 ? 2 : 0);
    R.texels += size_t(td.width) * td.height;
    if(R.texels > 0xffffffffull)
      return records_fail(err, "texture pool exceeds 2^32 texels");
  }
  if(d->numTextures == 0)
  {  // a 1x1 white default like src/scene.cpp:513-519
    R.texRecs[0] = TexRec{0, 1, 1, PT_FILTER_LINEAR, PT_WRAP_REPEAT, PT_WRAP_REPEAT, 3, 0};
    R.texels     = 1;
  }
  // ---- material lines, and the interleaved groups their descriptors point into.  The textures a material samples with one (u, v) -- normal, emissive,
  // metallic-roughness, base colour -- are ALSO stored texel by texel next to each other when they share size and sampler (the first present one sets the
  // shape): the 2 x 2 footprints of a shading's taps then share cache lines instead of pulling one or two 128-byte lines per texture for 16 bytes of texels
  // each (k_shade is the kernel next to the read-bandwidth ceiling).  Texel values and filter arithmetic are untouched; the plain copies stay for the any-hit
  // evaluation and the other texture roles.  PT_TUNE texGroups=0: descriptors point at the plain copies.
  R.matLines.assign(size_t(PT_MAT_LINE_QUADS) * std::max<size_t>(1, d->numMaterials), uint4{0u, 0u, 0u, 0u});
  for(uint32_t m = 0; m < d->numMaterials; ++m)
  {
    const pt_GltfShadeMaterial& mt = d->materials[m];
    const int ids[4] = {mt.normalTexture, mt.emissiveTexture, mt.pbrMetallicRoughnessTexture, mt.pbrBaseColorTexture};
    TexRec    rec[4];
    for(int k = 0; k < 4; ++k)
      rec[k] = R.texRecs[ids[k] > -1 ? size_t(ids[k]) : 0];
    SceneRecords::TexGroup g{{-1, -1, -1, -1}, 0, 0u};
    if(texGroups && d->numTextures)
      for(int k = 0; k < 4; ++k)
      {
        if(ids[k] < 0 || std::find(g.tex, g.tex + g.layers, ids[k]) != g.tex + g.layers)
          continue;
        const TexRec &a = R.texRecs[size_t(ids[k])], &b = R.texRecs[size_t(g.layers ? g.tex[0] : ids[k])];
        if(a.w == b.w && a.h == b.h && a.mag == b.mag && a.wrapS == b.wrapS && a.wrapT == b.wrapT)
          g.tex[g.layers++] = ids[k];
      }
    if(g.layers >= 2)
    {
      size_t at = R.groups.size();
      for(size_t q = 0; q < R.groups.size(); ++q)
        if(std::equal(g.tex, g.tex + 4, R.groups[q].tex))
          at = q;
      if(at == R.groups.size())
      {
        // the interleaved copy is an EXTRA on top of the plain copies (which serve the any-hit evaluation and the other texture roles): a group that
        // would take the pool past 2^32 texels is simply not made -- its material reads the plain copies, as with texGroups=0
        const TexRec& sh    = R.texRecs[size_t(g.tex[0])];
        const size_t  start = (R.texels + 31u) & ~size_t(31), after = start + size_t(sh.w) * sh.h * size_t(g.layers);
        if(after > 0xffffffffull)
        {
          mat_line_pack(mt, rec, &R.matLines[size_t(PT_MAT_LINE_QUADS) * m]);
          continue;
        }
        g.offset = uint32_t(start);
        R.texels = after;
        R.groups.push_back(g);
      }
      const SceneRecords::TexGroup& G = R.groups[at];
      for(int k = 0; k < 4; ++k)
      {
        const int* hit = ids[k] < 0 ? G.tex + G.layers : std::find(G.tex, G.tex + G.layers, ids[k]);
        if(hit == G.tex + G.layers)
          continue;  // absent, or of another shape: its plain copy
        rec[k].offset = G.offset;
        rec[k].tiled  = (rec[k].tiled & 1) | ((G.layers - 1) << 8) | (int(hit - G.tex) << 10);
      }
    }
    mat_line_pack(mt, rec, &R.matLines[size_t(PT_MAT_LINE_QUADS) * m]);
  }
  // ---- compact alpha view of every material (what the any-hit evaluation reads)
  R.alphaMats.assign(d->numMaterials, AlphaMat{});
  for(uint32_t m = 0; m < d->numMaterials; ++m)
  {
    const pt_GltfShadeMaterial& mt = d->materials[m];
    AlphaMat&                   a  = R.alphaMats[m];
    std::memset(&a, 0, sizeof(a));
    a.factorA = mt.pbrBaseColorFactor[3];
    a.cutoff  = mt.alphaCutoff;
    a.mode    = mt.alphaMode;
    a.tex     = mt.pbrBaseColorTexture;
    for(int k = 0; k < 8; ++k)
      a.m[k] = mt.uvTransform[k];
    a.mapOffset = ALPHA_NO_MAP;
    if(mt.pbrBaseColorTexture > -1)
    {
      const TexRec& tr = R.texRecs[mt.pbrBaseColorTexture];
      a.texOffset = tr.offset; a.texW = tr.w; a.texH = tr.h; a.texMag = tr.mag; a.texWrap = tr.wrapS | (tr.wrapT << 8) | (tr.pot << 16);
      if(tr.wrapS == PT_WRAP_REPEAT && tr.wrapT == PT_WRAP_REPEAT && tr.pot == 3)
        a.texWrap |= ALPHA_FAST_TAP;
      if(tr.tiled)
        a.texWrap |= ALPHA_TILED;
    }
  }
  build_opacity_maps(d, R.alphaMats, R.alphaMaps);
  return PT_OK;
}

// Where k_tail takes over (flush_pending): the first bounce whose queue is expected to hold <= tailBelow paths (maxDepth: never).
// Expectation = this launch's paths x the alive fraction observed at that bounce (ratio[0 .. numObserved), from the newest finished launch
// sequence); bounces beyond the observed ones continue the last observed shrink factor; before anything was observed a shrink of 0.3 per bounce
// is assumed (Russian roulette from depth 0 gives ~0.25 on the stand-in scenes).  A wrong guess costs time, never results.
int tail_from_depth(double paths, int maxDepth, int tailBelow, const double* ratio, int numObserved)
{
  if(tailBelow <= 0)
    return maxDepth;
  double r = 1.0, step = 0.3;
  for(int d = 0; d < maxDepth; ++d)
  {
    if(d < numObserved)
    {
      if(d > 0 && ratio[d - 1] > 0.0)
        step = std::min(1.0, ratio[d] / ratio[d - 1]);
      r = ratio[d];
    }
    else if(d > 0)
      r *= step;
    if(paths * r <= double(tailBelow))
      return d;
  }
  return maxDepth;
}

// PT_TUNE -> PtTuning, key by key (pt_internal.h)
void pt_parse_tuning(const char* tune, PtTuning& t, std::string& unknown)
{
  if(!tune)
    return;
  struct Key { const char* name; int PtTuning::*field; };
  static const Key keys[] = {{"stateMB", &PtTuning::stateMB}, {"stateGB", &PtTuning::stateGB}, {"packetClosest", &PtTuning::packetClosestBounces}, {"mergeSingles", &PtTuning::mergeSingles},
                             {"cnodes", &PtTuning::cnodes}, {"shadeTris", &PtTuning::shadeTris}, {"tail", &PtTuning::tailBelow}, {"warm", &PtTuning::warm}, {"texTile", &PtTuning::texTile},
                             {"texGroups", &PtTuning::texGroups}, {"regen", &PtTuning::regen}, {"packetTwo", &PtTuning::packetTwo}, {"blasWorkers", &PtTuning::blasWorkers},
                             {"batch", &PtTuning::batch}, {"inflight", &PtTuning::framesInFlight}, {"displaySlots", &PtTuning::displaySlots}, {"bands", &PtTuning::bands},
                             {"bandTiles", &PtTuning::bandTiles}, {"fuse", &PtTuning::fuse}, {"arena", &PtTuning::arena}, {"handover", &PtTuning::handover}, {"packetOrder", &PtTuning::packetOrder}};
  const std::string all(tune);
  size_t            at = 0;
  while(at <= all.size())
  {
    size_t end = all.find(',', at);
    if(end == std::string::npos)
      end = all.size();
    std::string tok = all.substr(at, end - at);
    at              = end + 1;
    while(!tok.empty() && (tok.front() == ' ' || tok.front() == '\t'))
      tok.erase(tok.begin());
    while(!tok.empty() && (tok.back() == ' ' || tok.back() == '\t'))
      tok.pop_back();
    if(tok.empty())
      continue;
    const size_t      eq  = tok.find('=');
    const std::string key = tok.substr(0, eq), val = eq == std::string::npos ? std::string() : tok.substr(eq + 1);
    bool              ok  = false;
    if(key == "build")
    {
      ok = true;
      if(val == "lbvh") t.sahBuild = PT_BUILD_LBVH;
      else if(val == "sah") t.sahBuild = PT_BUILD_SAH;
      else if(val == "ploc") t.sahBuild = PT_BUILD_PLOC;
      else if(val == "sahdev") t.sahBuild = PT_BUILD_SAHDEV;
      else ok = false;
    }
    else if(key == "accel")
    {
      ok = val == "two" || val == "flat";
      if(ok)
        t.accelTwoLevel = val == "two" ? 1 : 0;
    }
    else
      for(const Key& k : keys)
        if(key == k.name)
        {
          char*      e = nullptr;
          const long v = std::strtol(val.c_str(), &e, 10);
          if(!val.empty() && e && *e == 0)
          {
            t.*(k.field) = int(v);
            ok           = true;
          }
          break;
        }
    if(!ok)
      unknown += (unknown.empty() ? "" : ",") + tok;
  }
  if(t.bandTiles < 1)
    t.bandTiles = 1;
}

// test hook (no GPU involved): parses `tune` as pt_create would and reports the knobs in the order of the keys below plus build / accel / arena;
// `unknown` receives the tokens that name no knob.  Returns the number of values written.
extern "C" __attribute__((visibility("default"))) int pt_debug_parse_tuning(const char* tune, int* out, int maxOut, char* unknownOut, size_t unknownLen)
{
  PtTuning    t;
  std::string unknown;
  pt_parse_tuning(tune, t, unknown);
  const int v[] = {t.stateMB, t.stateGB, t.packetClosestBounces, t.mergeSingles, t.cnodes, t.shadeTris, t.tailBelow, t.warm, t.texTile, t.texGroups, t.regen, t.packetTwo,
                   t.blasWorkers, t.batch, t.framesInFlight, t.displaySlots, t.bands, t.bandTiles, t.fuse, t.sahBuild, t.accelTwoLevel, t.arena};
  const int n   = int(sizeof(v) / sizeof(v[0]));
  for(int i = 0; i < n && i < maxOut; ++i)
    out[i] = v[i];
  if(unknownOut && unknownLen)
    snprintf(unknownOut, unknownLen, "%s", unknown.c_str());
  return n < maxOut ? n : maxOut;
}

// the records of `d` with the knobs a context created now would get; a failure's message goes to `err`
static int debug_records(const pt_SceneDesc* d, SceneRecords& R, char* err, size_t errLen)
{
  std::string msg, unknown;
  PtTuning    tune;
  pt_parse_tuning(getenv("PT_TUNE"), tune, unknown);
  const int rc = build_scene_records(d, R, msg, tune.texTile, tune.texGroups);
  if(rc != PT_OK && err && errLen)
    snprintf(err, errLen, "%s", msg.c_str());
  return rc;
}
// Test hook (not part of the ABI; tests/cpp/trace_host.cpp): the host-side records pt_set_scene derives from a scene description, copied into
// caller arrays (no GPU involved).  Call with null outputs to get the counts: counts[0] instances, [1] materials, [2] opacity-map words,
// [3] texels of the RGBA8 pool, [4] world triangles.  instOut: InstanceRec[counts[0]] (128 B each); padOut: 2 floats per instance
// (TlasLeaf::padC0 / padC1 of the two-level walk); alphaMatsOut: AlphaMat[counts[1]] (80 B each); texelsOut: the pool in upload order;
// texRecsOut: TexRec[max(1, numTextures)] (32 B each).
extern "C" __attribute__((visibility("default"))) int pt_debug_scene_records(const pt_SceneDesc* d, unsigned long long* counts5, void* instOut, float* padOut, void* alphaMatsOut,
                                                                            uint32_t* alphaMapsOut, uint32_t* texelsOut, void* texRecsOut, char* err, size_t errLen)
{
  SceneRecords R;
  const int    rc = debug_records(d, R, err, errLen);
  if(rc != PT_OK)
    return rc;
  if(counts5)
  {
    counts5[0] = R.inst.size(); counts5[1] = R.alphaMats.size(); counts5[2] = R.alphaMaps.size(); counts5[3] = R.texels; counts5[4] = R.triTotal;
  }
  if(instOut)
    std::memcpy(instOut, R.inst.data(), sizeof(InstanceRec) * R.inst.size());
  if(padOut)
    for(size_t i = 0; i < R.inst.size(); ++i)
      two_level_pad(R.inst[i], R.primBound[R.inst[i].primMesh], padOut[2 * i], padOut[2 * i + 1]);
  if(alphaMatsOut)
    std::memcpy(alphaMatsOut, R.alphaMats.data(), sizeof(AlphaMat) * R.alphaMats.size());
  if(alphaMapsOut)
    std::memcpy(alphaMapsOut, R.alphaMaps.data(), 4 * R.alphaMaps.size());
  if(texRecsOut)
    std::memcpy(texRecsOut, R.texRecs.data(), sizeof(TexRec) * R.texRecs.size());
  if(texelsOut)
  {
    if(d->numTextures == 0)
      texelsOut[0] = 0xffffffffu;
    for(uint32_t t = 0; t < d->numTextures; ++t)
      store_texture(texelsOut + R.texRecs[t].offset, R.texRecs[t], d->textures[t].rgba8);
    for(const SceneRecords::TexGroup& g : R.groups)
      store_group(texelsOut + g.offset, g, R.texRecs, d);
  }
  return PT_OK;
}
// ... and the material lines (PT_MAT_LINE_QUADS x 16 bytes per material) whose descriptors point into that pool
extern "C" __attribute__((visibility("default"))) int pt_debug_mat_lines(const pt_SceneDesc* d, void* linesOut, char* err, size_t errLen)
{
  SceneRecords R;
  const int    rc = debug_records(d, R, err, errLen);
  if(rc != PT_OK)
    return rc;
  if(linesOut)
    std::memcpy(linesOut, R.matLines.data(), sizeof(uint4) * R.matLines.size());
  return PT_OK;
}

// Test hook (not part of the ABI): the launch-policy decision of flush_pending on plain numbers
extern "C" __attribute__((visibility("default"))) int pt_debug_tail_from(double paths, int maxDepth, int tailBelow, const double* ratio, int numObserved)
{
  return tail_from_depth(paths, maxDepth, tailBelow, ratio, numObserved);
}

// Test hook (not part of the ABI; CPU tests hold the bound to a float32 emulation of the ray transform): the instance record pt_set_scene
// derives from a node's world matrix and the object-space padding of the two-level walk for a mesh whose |coordinates| are <= Bo.
// out: objectToWorld rows (12), worldToObject rows (12), padC0, padC1, flags
extern "C" __attribute__((visibility("default"))) int pt_debug_two_level_pad(const float* worldMatrix16, float Bo, float* out27)
{
  InstanceRec I{};
  if(!worldMatrix16 || !out27 || !set_instance_transform(I, worldMatrix16, 0u))
    return PT_ERR_INVALID;
  const float4 rows[6] = {I.objectToWorld.r0, I.objectToWorld.r1, I.objectToWorld.r2, I.worldToObject.r0, I.worldToObject.r1, I.worldToObject.r2};
  for(int r = 0; r < 6; ++r)
  {
    out27[4 * r] = rows[r].x; out27[4 * r + 1] = rows[r].y; out27[4 * r + 2] = rows[r].z; out27[4 * r + 3] = rows[r].w;
  }
  two_level_pad(I, Bo, out27[24], out27[25]);
  out27[26] = float(I.flags);
  return PT_OK;
}
