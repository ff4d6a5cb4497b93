// The guide pass of the C++ shim (include/pt_renderer.hpp renderGuides / readDenoiseGuides) against the C ABI: compiles, links with libptmi.so and, with a
// GPU, renders the three planes of a quad, reads them back, and feeds the denoiser with them in place and re-installed -- with the same result.
// Without a GPU setup() must fail loudly (no fallback).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "stage/shim_common.h"

int main()
{
  ptmi::HipPathTracer r;
  r.setup(0);
  if(!r.ok())
    return shim_no_device(r);
  const float pos[12] = {-1, -1, 0, 1, -1, 0, 1, 1, 0, -1, 1, 0}, nrm[12] = {0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1};
  const float tan[16] = {1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1}, uv[8] = {0, 0, 1, 0, 1, 1, 0, 1};
  float       col[16];
  for(float& c : col) c = 1.f;
  pt_VertexAttributes v[4];
  pt_pack_vertices(4, pos, nrm, tan, uv, col, v);
  uint32_t             idx[6] = {0, 1, 2, 0, 2, 3};
  pt_PrimMesh          pm{0, 4, 0, 6, 0};
  pt_Node              nd{};
  for(int i = 0; i < 4; ++i) nd.worldMatrix[i * 5] = 1.f;
  pt_GltfShadeMaterial m{};
  m.pbrBaseColorFactor[0] = 0.75f; m.pbrBaseColorFactor[1] = 0.5f; m.pbrBaseColorFactor[2] = 0.25f;
  m.pbrBaseColorFactor[3] = 1.f;
  m.pbrBaseColorTexture = m.pbrMetallicRoughnessTexture = m.emissiveTexture = m.normalTexture = m.transmissionTexture = m.clearcoatTexture = m.clearcoatRoughnessTexture = m.thicknessTexture = -1;
  m.pbrRoughnessFactor = 1.f; m.ior = 1.5f; m.doubleSided = 0; m.attenuationDistance = 3.4e38f;
  m.attenuationColor[0] = m.attenuationColor[1] = m.attenuationColor[2] = 1.f;
  for(int i = 0; i < 4; ++i) m.uvTransform[i * 5] = 1.f;
  pt_SceneDesc sd{v, 4, idx, 6, &pm, 1, &nd, 1, &m, 1, nullptr, 0, nullptr, 0};
  const int    W = 24, H = 16;
  const size_t n = size_t(W) * H * 4;
  r.create({uint32_t(W), uint32_t(H)}, &sd);
  if(!r.ok())
  {
    std::printf("ERROR create: %s\n", r.lastError().c_str());
    return 4;
  }
  if(r.renderGuides() || r.status() != PT_ERR_STATE)  // before a camera exists
  {
    std::printf("ERROR renderGuides before setCamera: status %d\n", r.status());
    return 5;
  }
  const float    eye[3] = {0, 0, 3}, center[3] = {0, 0, 0}, up[3] = {0, 1, 0};
  pt_SceneCamera cam{};
  if(pt_camera_lookat(eye, center, up, 60.f, float(W) / float(H), &cam) != PT_OK)
    return 6;
  r.setCamera(cam);
  for(int mode : {PT_ACCEL_FLAT, PT_ACCEL_TWO_LEVEL})
  {
    r.setAccelMode(mode);
    std::vector<float> a(n, -1.f), nr(n, -1.f), d(n, -1.f);
    if(!r.renderGuides(PT_GUIDES_BASECOLOR | PT_GUIDES_NORMAL | PT_GUIDES_DEPTH, 50.f) || !r.readDenoiseGuides(a.data(), nr.data(), d.data()))
    {
      std::printf("ERROR renderGuides / readDenoiseGuides mode %d: %s\n", mode, r.lastError().c_str());
      return 7;
    }
    const size_t mid = (size_t(H / 2) * W + W / 2) * 4, corner = 0;  // the quad covers the middle of the image; the corners see past it
    const bool   hitOk = std::fabs(a[mid] - 0.75f) < 1e-6f && std::fabs(a[mid + 1] - 0.5f) < 1e-6f && std::fabs(a[mid + 2] - 0.25f) < 1e-6f && a[mid + 3] == 1.f && std::fabs(nr[mid] - 0.5f) < 1e-6f && std::fabs(nr[mid + 1] - 0.5f) < 1e-6f &&
                       std::fabs(nr[mid + 2] - 1.f) < 1e-6f && nr[mid + 3] == 1.f && std::fabs(d[mid] - 3.f) < 1e-2f && d[mid + 1] == 0.f && d[mid + 2] == 0.f && d[mid + 3] == 0.f;
    const bool   missOk = a[corner] == 0.f && a[corner + 3] == 1.f && nr[corner] == 0.f && nr[corner + 2] == 0.f && nr[corner + 3] == 1.f && d[corner] == 50.f && d[corner + 1] == 0.f;
    if(!hitOk || !missOk)
    {
      std::printf("ERROR mode %d: hit albedo %.3f %.3f %.3f normal %.3f %.3f %.3f depth %.3f; miss albedo %.3f normal %.3f depth %.3f\n", mode, a[mid], a[mid + 1], a[mid + 2], nr[mid],
                  nr[mid + 1], nr[mid + 2], d[mid], a[corner], nr[corner], d[corner]);
      return 8;
    }
    // the denoiser on the planes where the pass left them, and on the same planes installed by the caller
    std::vector<float> img(n), den0(n), den1(n);
    shim_image(img, 0);
    r.writeAccum(img.data());
    const pt_DenoiseParams p{3, 1.0f, {0.1f, 0.3f, 0.5f}, PT_DENOISE_DEMODULATE};
    if(!r.denoise(p, den0.data()) || !r.setDenoiseGuides(a.data(), nr.data(), d.data()) || !r.denoise(p, den1.data()) || std::memcmp(den0.data(), den1.data(), n * sizeof(float)) != 0)
    {
      std::printf("ERROR mode %d: denoise on rendered and on installed planes differs (%s)\n", mode, r.lastError().c_str());
      return 9;
    }
  }
  if(r.renderGuides(0u) || r.status() != PT_ERR_INVALID)
    return 10;
  std::printf("OK\n");
  return 0;
}
