// The temporal reprojection stage of the display path (the temporal half of SVGF, Schied et al. 2017; DESIGN.md section 5.3 is the definition): ONE
// output pixel of one call -- the current point of the pixel, its position in the history camera, the four-tap gather and the blend -- and what the
// host derives from pt_TemporalParams.  Plain inline functions of plain values, compiled by hipcc for the device (pt_temporal.hip) and by g++ for the
// host (tests/cpp/temporal_host.cpp), like pt_denoise.h: -ffp-contract=off, no fast math, no transcendental besides IEEE / and sqrtf, so that the
// device is held bit for bit to the host build and the host build to a float64 model of the definition.  No reference counterpart: the reference
// restarts its accumulation on every camera change.
//
// Where the values of a pixel come from is the caller's business (`Src`: row-major memory on the host, global memory on the device).
#pragma once
#include <math.h>
#include "pt_denoise.h"  // DnPx, dn_finite, dn_finite3, dn_dist2: the history shares the filter's notion of a finite colour and of normal distance

// What one call needs besides the images: the current camera's inverses (step 1), the history camera (step 2) and the checked parameters
struct TemporalConst {
  float viewInverse[16], projInverse[16];  // pt_SceneCamera of the current frame
  float worldToClipH[16];                  // forward matrix of the camera the history was made with
  float eyeH[3];                           // column 3 of that camera's viewInverse
  int   haveHistory;                       // 0: first call, or after a reset -- no pixel has history
  float depthTol, normalDist2, maxHistory;
};

// the four outcomes of step 4, in the order of the table of DESIGN.md section 5.3
enum { PT_TEMPORAL_BLEND = 0, PT_TEMPORAL_HISTORY_ONLY = 1, PT_TEMPORAL_CURRENT = 2, PT_TEMPORAL_NOTHING = 3 };

struct TemporalOut {
  DnPx  colour;  // out = Hc'
  DnPx  guide;   // Hg' = (g1.xyz, t)
  float length;  // Hn'
};
// what a test may look at besides the result (tests/cpp/temporal_host.cpp); the device passes no probe
struct TemporalProbe {
  float fx, fy;      // NaN where step 2 ended before they were formed
  int   tapX[4], tapY[4];
  int   verdict[4];  // 0: not looked at; 1: counted; 2: outside the image; 3: Hn < 1; 4: colour not finite; 5: depth; 6: normal
  float sw;
  int   outcome;     // PT_TEMPORAL_*
  float P[3], tExp;
};

// PT_OK, or why the parameters cannot be used (`why`: static text)
PT_DN int temporal_constants(const pt_TemporalParams* p, const char** why)
{
  if(!p)
    return *why = "null parameters", PT_ERR_INVALID;
  for(int i = 0; i < 16; ++i)
    if(!dn_finite(p->worldToClip[i]))
      return *why = "worldToClip has an entry that is not finite", PT_ERR_INVALID;
  if(!(p->depthTol > 0.0f) || !dn_finite(p->depthTol))
    return *why = "depthTol must be positive and finite", PT_ERR_INVALID;
  if(!(p->normalDist2 >= 0.0f) || !dn_finite(p->normalDist2))
    return *why = "normalDist2 must be non-negative and finite", PT_ERR_INVALID;
  if(!(p->maxHistory >= 1.0f) || !dn_finite(p->maxHistory))
    return *why = "maxHistory must be at least 1 and finite", PT_ERR_INVALID;
  if(p->flags != 0u)
    return *why = "unknown flag bits", PT_ERR_INVALID;
  return PT_OK;
}

// The constants of one call: the current camera's two inverses, the camera the history was made with (worldToClipH[16] and eyeH[3]; both NULL: there is
// no history and the fields stay zero) and parameters temporal_constants accepted.  The one place that fills a TemporalConst, for the device path
// (pt_temporal.hip) and the host builds (tests/cpp/temporal_host.cpp, svgf_host.cpp) alike; words are copied as they are.
PT_DN TemporalConst temporal_const(const float* viewInverse, const float* projInverse, const float* worldToClipH, const float* eyeH, const pt_TemporalParams* p)
{
  TemporalConst k{};
  for(int i = 0; i < 16; ++i)
  {
    k.viewInverse[i] = viewInverse[i];
    k.projInverse[i] = projInverse[i];
    if(worldToClipH)
      k.worldToClipH[i] = worldToClipH[i];
  }
  for(int i = 0; i < 3 && eyeH; ++i)
    k.eyeH[i] = eyeH[i];
  k.haveHistory = worldToClipH && eyeH ? 1 : 0;
  k.depthTol    = p->depthTol;
  k.normalDist2 = p->normalDist2;
  k.maxHistory  = p->maxHistory;
  return k;
}

// row r of mat4_mul (pt_shade.h): ((c0 * v.x + c1 * v.y) + c2 * v.z) + c3 * v.w for the column-major m
PT_DN float tp_mat4_row(const float* m, int r, float x, float y, float z, float w) { return ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * w; }
PT_DN float tp_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }  // dot3 of pt_math.h
PT_DN float tp_mix(float a, float b, float t) { return a * (1.0f - t) + b * t; }                                        // lerp of pt_math.h (GLSL mix)

// the point steps 2 and 3 run on
struct TemporalPoint {
  float Px, Py, Pz;
};

// Step 1 for pixel (px, py) of a w x h image whose depth plane holds t there, as a statement sequence over the names k, px, py, w, h and t that leaves
// the current eye in ox, oy, oz and the current point in Px, Py, Pz.  Stated once and expanded in temporal_pixel below and in temporal_pixel_moving
// (pt_motion.h).  A macro and not a function: with step 1 in a function of its own -- by value, by reference, returning the point or writing it -- the
// kernels of pt_temporal.hip and pt_svgf.hip compile to other device code than before (the vectoriser pairs step 1's products differently: 151
// differing lines of assembly in k_temporal), whereas the expansion leaves every line of them as it was (tools/device_code_diff.sh).
#define PT_TEMPORAL_STEP_1 \
  /* step 1: the pinhole half of camera_ray (pt_shade.h), jitter (0.5, 0.5), no lens */                                                \
  const float cx = float(px) + 0.5f, cy = float(py) + 0.5f;                                                                            \
  const float ux = cx / float(w), uy = cy / float(h);                                                                                  \
  const float dx = ux * 2.0f - 1.0f, dy = uy * 2.0f - 1.0f;                                                                            \
  const float ox = tp_mat4_row(k.viewInverse, 0, 0.0f, 0.0f, 0.0f, 1.0f), oy = tp_mat4_row(k.viewInverse, 1, 0.0f, 0.0f, 0.0f, 1.0f),  \
              oz = tp_mat4_row(k.viewInverse, 2, 0.0f, 0.0f, 0.0f, 1.0f);                                                              \
  const float tx = tp_mat4_row(k.projInverse, 0, dx, dy, 1.0f, 1.0f), ty = tp_mat4_row(k.projInverse, 1, dx, dy, 1.0f, 1.0f),          \
              tz = tp_mat4_row(k.projInverse, 2, dx, dy, 1.0f, 1.0f);                                                                  \
  const float tinv = 1.0f / sqrtf(tp_dot3(tx, ty, tz, tx, ty, tz)); /* unit() */                                                       \
  const float nx = tx * tinv, ny = ty * tinv, nz = tz * tinv;                                                                          \
  const float rx = tp_mat4_row(k.viewInverse, 0, nx, ny, nz, 0.0f), ry = tp_mat4_row(k.viewInverse, 1, nx, ny, nz, 0.0f),              \
              rz = tp_mat4_row(k.viewInverse, 2, nx, ny, nz, 0.0f);                                                                    \
  const float rinv = 1.0f / sqrtf(tp_dot3(rx, ry, rz, rx, ry, rz));                                                                    \
  const float Px = ox + (rx * rinv) * t, Py = oy + (ry * rinv) * t, Pz = oz + (rz * rinv) * t;

// Steps 2 to 4 for a pixel whose own values are c, g1 and t: `q` is the point steps 2 and 3 run on (step 1's, or what the motion table of section 5.5
// made of it: pt_motion.h) and gn the encoded normal the taps are tested against (g1, or the one sent through the table); step 4 and the stored guide
// take c, g1 and t as they are.  (ox, oy, oz): the current eye, which no step after the first reads.
template <class Src>
PT_DN void temporal_resolve(const Src& src, const TemporalConst& k, const DnPx& c, const DnPx& g1, float t, float ox, float oy, float oz, const TemporalPoint& q,
                                   const DnPx& gn, int w, int h, TemporalProbe* probe, TemporalOut& o)
{
  const float Px = q.Px, Py = q.Py, Pz = q.Pz;

  bool  history = false;
  float hr = 0.0f, hg = 0.0f, hb = 0.0f, N = 0.0f;
  if(probe)
  {
    probe->fx = probe->fy = nanf("");
    probe->sw = 0.0f;
    probe->P[0] = Px, probe->P[1] = Py, probe->P[2] = Pz;
    probe->tExp = nanf("");
    for(int i = 0; i < 4; ++i)
      probe->tapX[i] = probe->tapY[i] = probe->verdict[i] = 0;
  }
  if(k.haveHistory)
  {
    // step 2: where the history camera saw P, and at what depth
    const float clx = tp_mat4_row(k.worldToClipH, 0, Px, Py, Pz, 1.0f), cly = tp_mat4_row(k.worldToClipH, 1, Px, Py, Pz, 1.0f),
                clz = tp_mat4_row(k.worldToClipH, 2, Px, Py, Pz, 1.0f), clw = tp_mat4_row(k.worldToClipH, 3, Px, Py, Pz, 1.0f);
    const float ex = Px - k.eyeH[0], ey = Py - k.eyeH[1], ez = Pz - k.eyeH[2];
    const float tExp = sqrtf(tp_dot3(ex, ey, ez, ex, ey, ez));
    if(probe)
      probe->tExp = tExp;
    if(dn_finite(Px) && dn_finite(Py) && dn_finite(Pz) && dn_finite(clx) && dn_finite(cly) && dn_finite(clz) && dn_finite(clw) && dn_finite(tExp) && clw > 0.0f)
    {
      const float fx = ((clx / clw) * 0.5f + 0.5f) * float(w) - 0.5f;
      const float fy = ((cly / clw) * 0.5f + 0.5f) * float(h) - 0.5f;
      if(probe)
        probe->fx = fx, probe->fy = fy;
      if(fx > -1.0f && fx < float(w) && fy > -1.0f && fy < float(h))  // false for a NaN; only now are they converted
      {
        // step 3: the four taps
        const float x0f = floorf(fx), y0f = floorf(fy);
        const int   x0 = int(x0f), y0 = int(y0f);  // -1 .. w - 1, -1 .. h - 1
        const float wx = fx - x0f, wy = fy - y0f;
        const float wgt[4] = {(1.0f - wx) * (1.0f - wy), wx * (1.0f - wy), (1.0f - wx) * wy, wx * wy};
        float       sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f;
        for(int i = 0; i < 4; ++i)
        {
          const int qx = x0 + (i & 1), qy = y0 + (i >> 1);
          int       verdict;
          if(qx < 0 || qx >= w || qy < 0 || qy >= h)
            verdict = 2;
          else
          {
            const float hn = src.histLength(qx, qy);
            const DnPx  hc = src.histColour(qx, qy), hq = src.histGuide(qx, qy);
            if(!(hn >= 1.0f))
              verdict = 3;
            else if(!dn_finite3(hc))
              verdict = 4;
            else if(!(ptf_abs(hq.w - tExp) <= k.depthTol * tExp))
              verdict = 5;
            else if(!(dn_dist2(gn, hq) <= k.normalDist2))
              verdict = 6;
            else
            {
              verdict = 1;
              // a tap that does not count is left out, not added as 0
              sw = sw + wgt[i];
              sr = sr + wgt[i] * hc.x;
              sg = sg + wgt[i] * hc.y;
              sb = sb + wgt[i] * hc.z;
              sn = sn + wgt[i] * hn;
            }
          }
          if(probe)
            probe->tapX[i] = qx, probe->tapY[i] = qy, probe->verdict[i] = verdict;
        }
        if(probe)
          probe->sw = sw;
        if(sw > 0.0f)
        {
          history = true;
          hr = sr / sw, hg = sg / sw, hb = sb / sw;
          N = sn / sw;
        }
      }
    }
  }

  // step 4
  const bool  fin = dn_finite3(c);
  o.colour = c;  // alpha is the current pixel's in every case
  o.guide  = DnPx{g1.x, g1.y, g1.z, t};
  int outcome;
  if(history && fin)
  {
    const float n1 = N + 1.0f;
    const float Nn = k.maxHistory < n1 ? k.maxHistory : n1;  // GLSL min(N + 1, maxHistory)
    const float a  = 1.0f / Nn;
    o.colour.x = tp_mix(hr, c.x, a);
    o.colour.y = tp_mix(hg, c.y, a);
    o.colour.z = tp_mix(hb, c.z, a);
    o.length   = Nn;
    outcome    = PT_TEMPORAL_BLEND;
  }
  else if(history)
  {
    o.colour.x = hr, o.colour.y = hg, o.colour.z = hb;
    o.length   = N;
    outcome    = PT_TEMPORAL_HISTORY_ONLY;
  }
  else if(fin)
  {
    o.length = 1.0f;
    outcome  = PT_TEMPORAL_CURRENT;
  }
  else
  {
    o.length = 0.0f;  // never gathered; the spatial filter repairs the colour
    outcome  = PT_TEMPORAL_NOTHING;
  }
  if(probe)
    probe->outcome = outcome;
}

// Pixel (px, py) of a W x H image.  src.colour / src.normal / src.depth are the accumulation image and guide planes 1 and 2 at the pixel itself;
// src.histColour / src.histGuide / src.histLength are the history set that is READ, asked only for positions inside the image and only when
// k.haveHistory is set.  Every index formed here lies inside the image for every input bit pattern: the range tests of step 2 are float comparisons
// that a NaN fails and run before the conversion to int, and each tap is tested against the image again.
// Step 1 and steps 2 to 4 composed: the stage as section 5.3 defines it.
template <class Src>
PT_DN TemporalOut temporal_pixel(const Src& src, const TemporalConst& k, int px, int py, int w, int h, TemporalProbe* probe)
{
  const DnPx  c = src.colour(px, py), g1 = src.normal(px, py);
  const float t = src.depth(px, py).x;
  PT_TEMPORAL_STEP_1
  TemporalOut o;
  temporal_resolve(src, k, c, g1, t, ox, oy, oz, TemporalPoint{Px, Py, Pz}, g1, w, h, probe, o);
  return o;
}

// Src over row-major planes in ordinary memory (the host build; the device has its own reader with 16-byte loads)
struct TpRowMajor {
  const DnPx * c, *g1, *g2, *hc, *hg;
  const float* hn;
  int          w;
  PT_DN_MEMBER DnPx  colour(int x, int y) const { return c[size_t(y) * size_t(w) + size_t(x)]; }
  PT_DN_MEMBER DnPx  normal(int x, int y) const { return g1[size_t(y) * size_t(w) + size_t(x)]; }
  PT_DN_MEMBER DnPx  depth(int x, int y) const { return g2[size_t(y) * size_t(w) + size_t(x)]; }
  PT_DN_MEMBER DnPx  histColour(int x, int y) const { return hc[size_t(y) * size_t(w) + size_t(x)]; }
  PT_DN_MEMBER DnPx  histGuide(int x, int y) const { return hg[size_t(y) * size_t(w) + size_t(x)]; }
  PT_DN_MEMBER float histLength(int x, int y) const { return hn[size_t(y) * size_t(w) + size_t(x)]; }
};
