// Child order of a 4-wide node, decided when the node is built instead of per visit (pt_packet.h): one byte per direction-sign octant
// o = sx | sy << 1 | sz << 2 (bit set: the rays travel towards smaller coordinates on that axis), the four child slots nearest first at 2 bits each
// (the nearest in the low bits).  The sort key of a child is its box's entry corner projected on the octant's diagonal: the sum over the axes of
// `lo` where the rays travel up and `-hi` where they travel down, added as (x + y) + z in float.  Ties go by slot number, empty slots come last.
// The bytes are stored XOR PT_ORDER_SLOTS in the first 8 bytes of WideNode::pad (octants 0..3 in pad[0].x, 4..7 in pad[0].y), so that a zeroed pad
// decodes to slot order: a structure whose builder knows nothing of the table stays valid.  The order is a heuristic of the packet walk only; no
// result depends on it (trace contract: the candidate rules are independent of the visiting order).
// Plain C++, so that the collapse kernel (pt_accel.hip k_collapse) and the CPU test (tests/test_packet_order.py) run the same code.
#pragma once
#include "pt_device.h"

#if defined(__HIPCC__)
#define PO_FN __host__ __device__ inline
#else
#define PO_FN inline
#endif

#define PT_ORDER_SLOTS 0xE4u  // slots 0, 1, 2, 3 in this order

#if PT_BVH_WIDTH == 4
// lo / hi: the planes [axis][slot]; cc: the child references (BVH_NONE: empty slot).  out: the two words as stored
PO_FN void pt_order_encode(const float lo[3][4], const float hi[3][4], const uint32_t cc[4], uint32_t out[2])
{
  out[0] = out[1] = 0u;
  for(uint32_t o = 0; o < 8u; ++o)
  {
    float key[4];
    for(int k = 0; k < 4; ++k)
    {
      const float x = (o & 1u) ? -hi[0][k] : lo[0][k], y = (o & 2u) ? -hi[1][k] : lo[1][k], z = (o & 4u) ? -hi[2][k] : lo[2][k];
      key[k]        = (x + y) + z;
    }
    uint32_t ord[4] = {0u, 1u, 2u, 3u};
    for(int i = 1; i < 4; ++i)  // stable insertion sort: equal keys keep slot order
      for(int j = i; j > 0; --j)
      {
        const uint32_t a = ord[j], b = ord[j - 1];
        const bool     ea = cc[a] == BVH_NONE, eb = cc[b] == BVH_NONE;
        const bool     before = ea != eb ? eb : (!ea && key[a] < key[b]);
        if(!before)
          break;
        ord[j]     = b;
        ord[j - 1] = a;
      }
    const uint32_t byte = (ord[0] | (ord[1] << 2) | (ord[2] << 4) | (ord[3] << 6)) ^ PT_ORDER_SLOTS;
    out[o >> 2] |= byte << (8u * (o & 3u));
  }
}

// the decoded byte of octant o out of the two stored words
PO_FN uint32_t pt_order_byte(uint32_t w0, uint32_t w1, uint32_t o)
{
  return (((o & 4u) ? w1 : w0) >> (8u * (o & 3u)) & 0xffu) ^ PT_ORDER_SLOTS;
}

// writes the table of a finished node (planes and child references in place) into its pad
PO_FN void pt_order_write(WideNode& w)
{
  const float    lo[3][4] = {{w.minx[0].x, w.minx[0].y, w.minx[0].z, w.minx[0].w}, {w.miny[0].x, w.miny[0].y, w.miny[0].z, w.miny[0].w}, {w.minz[0].x, w.minz[0].y, w.minz[0].z, w.minz[0].w}};
  const float    hi[3][4] = {{w.maxx[0].x, w.maxx[0].y, w.maxx[0].z, w.maxx[0].w}, {w.maxy[0].x, w.maxy[0].y, w.maxy[0].z, w.maxy[0].w}, {w.maxz[0].x, w.maxz[0].y, w.maxz[0].z, w.maxz[0].w}};
  const uint32_t cc[4]    = {w.child[0].x, w.child[0].y, w.child[0].z, w.child[0].w};
  uint32_t       t[2];
  pt_order_encode(lo, hi, cc, t);
  w.pad[0].x = t[0];
  w.pad[0].y = t[1];
}
#endif
