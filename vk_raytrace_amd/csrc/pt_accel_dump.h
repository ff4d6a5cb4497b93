/* Read-back of a built acceleration structure for the tests (pt_debug_accel_info / pt_debug_accel_read in pt_debug.hip, th_accel_info /
   th_accel_read in tests/cpp/trace_host.cpp; judged by tests/accel_audit.py).  Plain C: array ids and the layout of the info record.  Not part of the ABI. */
#ifndef PT_ACCEL_DUMP_H
#define PT_ACCEL_DUMP_H

enum {
  PT_DUMP_WIDE = 0,        /* WideNode[]: flat structure, or the concatenated bottom-level structures */
  PT_DUMP_CNODES,          /* CompactNode[], same numbering (haveCNodes) */
  PT_DUMP_TRIS,            /* TriRec[], leaf order */
  PT_DUMP_ALPHA_RECS,      /* AlphaRec[], parallel to TRIS */
  PT_DUMP_BVH2,            /* BvhNode[]: flat structure only */
  PT_DUMP_TLAS,            /* WideNode[] of the instance hierarchy */
  PT_DUMP_CTLAS,           /* CompactNode[] of it */
  PT_DUMP_TLAS_LEAVES,     /* TlasLeaf[] */
  PT_DUMP_INST_TRI_BASE,   /* uint32 per instance */
  PT_DUMP_INST_BLOCK,      /* uint32[(numTris >> PT_INST_BLOCK_SHIFT) + 2] */
  PT_DUMP_INST_NODE_BASE,  /* uint32 per instance (host copy) */
  PT_DUMP_INST_PAD,        /* 2 floats per instance */
  PT_DUMP_ACTIVE,          /* uint32 per active instance */
  PT_DUMP_BLAS_RANGES,     /* (node base, wide nodes) per object-space BLAS (host copy) */
  PT_DUMP_MERGED_LIST,     /* instances of the merged world-space structure (host copy) */
  PT_DUMP_SHADE_TRIS,      /* PT_SHADE_REC_QUADS float4 per leaf slot (haveShadeTris) */
  PT_DUMP_COUNT
};

/* the info record: uint32 words */
enum {
  PT_DUMPI_ACCEL_MODE = 0,
  PT_DUMPI_NUM_TRIS,
  PT_DUMPI_NUM_INSTANCES,
  PT_DUMPI_NUM_WIDE_NODES,
  PT_DUMPI_NODE_CAPACITY,
  PT_DUMPI_NUM_BVH_NODES,
  PT_DUMPI_NUM_TLAS_NODES,
  PT_DUMPI_NUM_ACTIVE,
  PT_DUMPI_NUM_BLAS,
  PT_DUMPI_MERGED_TRIS,
  PT_DUMPI_MERGED_WIDE,
  PT_DUMPI_MERGED_ONLY,
  PT_DUMPI_HAVE_CNODES,
  PT_DUMPI_HAVE_SHADE_TRIS,
  PT_DUMPI_MERGED_BOX,     /* six words: lo.xyz, hi.xyz as float bits */
  PT_DUMPI_BUILDER = PT_DUMPI_MERGED_BOX + 6,  /* PT_TUNE build= in force (PtBuilder) */
  PT_DUMPI_WORDS
};

#endif
