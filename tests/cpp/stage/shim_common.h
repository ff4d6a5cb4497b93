// What the *_shim_test.cpp programs share: the line and exit status of a setup() without a device, the checksum, the planes and images of the rounds that
// tests/shim.py builds word for word on the Python side, and the display pass's default settings.
#pragma once
#include <cstdio>
#include <vector>
#include "pt_renderer.hpp"

// setup() did not succeed: says so, and is the program's exit status -- 0 only where the reason is that there is no device (no fallback)
inline int shim_no_device(ptmi::HipPathTracer& r)
{
  std::printf("NO_DEVICE status=%d msg=%s\n", r.status(), r.lastError().c_str());
  return r.status() == PT_ERR_NO_DEVICE ? 0 : 3;
}

// FNV-1a over the bytes (tests/shim.py fnv)
inline unsigned long long fnv(const void* p, size_t bytes)
{
  unsigned long long   h = 1469598103934665603ull;
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for(size_t i = 0; i < bytes; ++i)
    h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

// guide planes 1 and 2 of a w x h image (tests/shim.py planes): one encoded normal everywhere, depths 4 .. 5.875 in steps of 1/8
inline void shim_planes(int w, int h, std::vector<float>& normal, std::vector<float>& depth)
{
  normal.assign(size_t(w) * h * 4, 0.f);
  depth.assign(size_t(w) * h * 4, 0.f);
  for(int y = 0; y < h; ++y)
    for(int x = 0; x < w; ++x)
    {
      const size_t at = (size_t(y) * w + x) * 4;
      normal[at] = 0.5f, normal[at + 1] = 0.5f, normal[at + 2] = 1.f, normal[at + 3] = 1.f;
      depth[at] = 4.f + float((x * 3 + y * 5) % 16) * 0.125f;
    }
}

// image k of a round (tests/shim.py image): word i is (i (37 + 4 k)) mod 101 / 50
inline void shim_image(std::vector<float>& img, int k)
{
  for(size_t i = 0; i < img.size(); ++i)
    img[i] = float((i * (37u + 4u * unsigned(k))) % 101u) / 50.f;
}

// host_device.default_tonemapper()
inline pt_Tonemapper shim_tonemapper()
{
  pt_Tonemapper tm{};
  tm.brightness = 1.f, tm.contrast = 1.f, tm.saturation = 1.f, tm.vignette = 0.f, tm.avgLum = 1.f, tm.zoom = 1.f, tm.renderingRatio[0] = tm.renderingRatio[1] = 1.f;
  tm.autoExposure = 0, tm.Ywhite = 0.5f, tm.key = 0.5f, tm.dither = 1;
  return tm;
}
