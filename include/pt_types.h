/*
 * pt_types.h -- plain-C mirror of the structures the reference shares between
 * host and device (reference: shaders/host_device.h:107-281), plus the flat
 * scene description that replaces the reference's descriptor sets at the
 * drop-in boundary (reference: shaders/layouts.glsl:37-52).
 *
 * Layout rule: scalar block layout == packed C with 4-byte alignment.
 * All matrices are column-major (element [col*4 + row]) like GLSL / glm.
 * Sizes are asserted below; SURVEY.md Appendix A lists the dword offsets.
 */
#ifndef PT_TYPES_H
#define PT_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_TILE 32 /* framebuffer tile edge in pixels (multi-GPU shard granularity) */

/* reference: shaders/host_device.h:88-102 (DebugMode) */
enum pt_DebugMode {
  PT_DEBUG_NONE = 0,
  PT_DEBUG_BASECOLOR = 1,
  PT_DEBUG_NORMAL = 2,
  PT_DEBUG_METALLIC = 3,
  PT_DEBUG_EMISSIVE = 4,
  PT_DEBUG_ALPHA = 5,
  PT_DEBUG_ROUGHNESS = 6,
  PT_DEBUG_TEXCOORD = 7,
  PT_DEBUG_TANGENT = 8,
  PT_DEBUG_RADIANCE = 9,
  PT_DEBUG_WEIGHT = 10,
  PT_DEBUG_RAYDIR = 11,
  PT_DEBUG_HEATMAP = 12
};

/* reference: shaders/host_device.h:126-131 */
enum { PT_ALPHA_OPAQUE = 0, PT_ALPHA_MASK = 1, PT_ALPHA_BLEND = 2 };
/* reference: shaders/host_device.h:211-213 */
enum { PT_LIGHT_DIRECTIONAL = 0, PT_LIGHT_POINT = 1, PT_LIGHT_SPOT = 2 };

/* reference: shaders/host_device.h:183-196 -- the per-frame kernel config (was a push constant) */
typedef struct pt_RtxState {
  int32_t frame;
  int32_t maxDepth;
  int32_t maxSamples;
  float   fireflyClampThreshold;
  float   hdrMultiplier;
  int32_t debugging_mode;
  int32_t pbrMode; /* 0 Disney, 1 glTF */
  int32_t _pad0;
  int32_t size[2];
  int32_t minHeatmap;
  int32_t maxHeatmap;
} pt_RtxState;

/* reference: shaders/host_device.h:107-115 */
typedef struct pt_SceneCamera {
  float   viewInverse[16];
  float   projInverse[16];
  float   focalDist;
  float   aperture;
  int32_t nbLights;
} pt_SceneCamera;

/* reference: shaders/host_device.h:117-124 */
typedef struct pt_VertexAttributes {
  float    position[3];
  uint32_t normal;      /* 16+16 bit octahedral */
  float    texcoord[2]; /* LSB of texcoord[1] = tangent handedness */
  uint32_t tangent;     /* 16+16 bit octahedral */
  uint32_t color;       /* RGBA8 unorm */
} pt_VertexAttributes;

/* reference: shaders/host_device.h:133-179 */
typedef struct pt_GltfShadeMaterial {
  float   pbrBaseColorFactor[4];
  int32_t pbrBaseColorTexture;
  float   pbrMetallicFactor;
  float   pbrRoughnessFactor;
  int32_t pbrMetallicRoughnessTexture;
  int32_t emissiveTexture;
  int32_t _pad0;
  float   emissiveFactor[3];
  int32_t alphaMode;
  float   alphaCutoff;
  int32_t doubleSided;
  int32_t normalTexture;
  float   normalTextureScale;
  float   uvTransform[16];
  int32_t unlit;
  float   transmissionFactor;
  int32_t transmissionTexture;
  float   ior;
  float   anisotropyDirection[3];
  float   anisotropy;
  float   attenuationColor[3];
  float   thicknessFactor;
  int32_t thicknessTexture;
  float   attenuationDistance;
  float   clearcoatFactor;
  float   clearcoatRoughness;
  int32_t clearcoatTexture;
  int32_t clearcoatRoughnessTexture;
  uint32_t sheen;
  int32_t _pad1;
} pt_GltfShadeMaterial;

/* reference: shaders/host_device.h:215-230 */
typedef struct pt_Light {
  float   direction[3];
  float   range;
  float   color[3];
  float   intensity;
  float   position[3];
  float   innerConeCos;
  float   outerConeCos;
  int32_t type;
  float   padding[2];
} pt_Light;

/* reference: shaders/host_device.h:233-239 */
typedef struct pt_EnvAccel {
  uint32_t alias;
  float    q;
  float    pdf;
  float    aliasPdf;
} pt_EnvAccel;

/* reference: shaders/host_device.h:242-255 */
typedef struct pt_Tonemapper {
  float   brightness;
  float   contrast;
  float   saturation;
  float   vignette;
  float   avgLum;
  float   zoom;
  float   renderingRatio[2];
  int32_t autoExposure;
  float   Ywhite;
  float   key;
  int32_t dither;
} pt_Tonemapper;

/* reference: shaders/host_device.h:258-281 */
typedef struct pt_SunAndSky {
  float   rgb_unit_conversion[3];
  float   multiplier;
  float   haze;
  float   redblueshift;
  float   saturation;
  float   horizon_height;
  float   ground_color[3];
  float   horizon_blur;
  float   night_color[3];
  float   sun_disk_intensity;
  float   sun_direction[3];
  float   sun_disk_scale;
  float   sun_glow_intensity;
  int32_t y_is_up;
  int32_t physically_scaled_sun;
  int32_t in_use;
} pt_SunAndSky;

/* ---- flat scene description (replaces descriptor sets 0 and 2) ---------------------------- */

/* One glTF primitive == one BLAS in the reference (src/accelstruct.cpp:110-127,
 * nvh::GltfPrimMesh fields used at src/scene.cpp:205-252).  Indices are relative
 * to vertexOffset, exactly as the reference's per-primitive index buffers are. */
typedef struct pt_PrimMesh {
  uint32_t vertexOffset;
  uint32_t vertexCount;
  uint32_t firstIndex;
  uint32_t indexCount;
  int32_t  materialIndex;
} pt_PrimMesh;

/* One glTF node == one TLAS instance in the reference (src/accelstruct.cpp:137-159). */
typedef struct pt_Node {
  float   worldMatrix[16]; /* column-major object->world */
  int32_t primMesh;        /* == instanceCustomIndex */
} pt_Node;

/* Sampler state as it reaches the shader (VkFilter / VkSamplerAddressMode numeric values;
 * reference: src/scene.cpp:447-482,561-571). Only the mag filter matters: every tap is LOD 0. */
/* the reference's two Renderer implementations (src/sample_example.hpp:136-137), see pt_set_variant */
enum { PT_VARIANT_RAYQUERY = 0, PT_VARIANT_RTX = 1 };
/* layout of the acceleration structure, see pt_set_accel_mode */
enum { PT_ACCEL_FLAT = 0, PT_ACCEL_TWO_LEVEL = 1 };
/* functions of the fp32 transcendental contract (pt_fpmath.h), for pt_fpmath_eval */
enum { PT_FN_SIN = 0, PT_FN_COS, PT_FN_TAN, PT_FN_ASIN, PT_FN_ACOS, PT_FN_ATAN2, PT_FN_EXP, PT_FN_LOG, PT_FN_POW };
enum { PT_FILTER_NEAREST = 0, PT_FILTER_LINEAR = 1 };
enum { PT_WRAP_REPEAT = 0, PT_WRAP_MIRRORED_REPEAT = 1, PT_WRAP_CLAMP_TO_EDGE = 2 };

typedef struct pt_TextureDesc {
  const uint8_t* rgba8; /* width*height*4, row 0 first (R8G8B8A8_UNORM, src/scene.cpp:493) */
  int32_t        width;
  int32_t        height;
  int32_t        magFilter;
  int32_t        minFilter;
  int32_t        wrapS;
  int32_t        wrapT;
} pt_TextureDesc;

typedef struct pt_SceneDesc {
  const pt_VertexAttributes*  vertices;
  uint32_t                    numVertices;
  const uint32_t*             indices;
  uint32_t                    numIndices;
  const pt_PrimMesh*          primMeshes;
  uint32_t                    numPrimMeshes;
  const pt_Node*              nodes;
  uint32_t                    numNodes;
  const pt_GltfShadeMaterial* materials;
  uint32_t                    numMaterials;
  const pt_Light*             lights; /* may be NULL when numLights == 0 */
  uint32_t                    numLights;
  const pt_TextureDesc*       textures; /* may be NULL when numTextures == 0 */
  uint32_t                    numTextures;
} pt_SceneDesc;

/* Result of pt_pick: the fields of nvvk::RayPickerKHR::PickResult the reference consumes (src/sample_example.cpp:493-510). */
typedef struct pt_PickResult {
  float    worldRayOrigin[3];
  float    hitT;               /* distance along the ray; undefined when nothing is hit */
  float    worldRayDirection[3];
  int32_t  primitiveID;        /* triangle inside the prim-mesh */
  uint32_t instanceID;         /* node (TLAS instance) index, 0xffffffff: nothing hit */
  int32_t  instanceCustomIndex;/* prim-mesh index */
  float    baryCoord[3];       /* (1 - u - v, u, v) */
} pt_PickResult;

/* pt_trace_rays: one ray in, hits_per_ray results out (32 bytes each).  The ray kinds are pieces of the trace contract (DESIGN.md section 3,
 * "Ray queries"); what every field means per kind is stated at pt_trace_rays in pt_api.h. */
typedef struct pt_Ray {
  float    origin[3];
  float    tmax;       /* exclusive upper bound of t for the bounded kinds (ignored by PT_RAYS_CLOSEST); <= 0: empty range, a plain miss */
  float    direction[3]; /* not normalised by the library: t is in units of its length */
  uint32_t seed;       /* RNG state before the ray's alpha draws */
} pt_Ray;
typedef struct pt_RayHit {
  float    t, u, v;              /* hit distance and barycentrics (weights 1 - u - v, u, v); 0 on a miss */
  uint32_t instanceID;           /* node (TLAS instance) index as in pt_PickResult, 0xffffffff: miss */
  int32_t  primitiveID;          /* triangle inside the prim-mesh, -1: miss */
  int32_t  instanceCustomIndex;  /* prim-mesh index, -1: miss */
  uint32_t seed;                 /* RNG state after the ray's alpha draws (the input where the kind draws nothing) */
  uint32_t status;               /* PT_RAY_HIT | PT_RAY_INVALID */
} pt_RayHit;
enum { PT_RAYS_CLOSEST = 0, PT_RAYS_OCCLUDED = 1, PT_RAYS_NEAREST = 2, PT_RAYS_CANDIDATES = 3 }; /* pt_trace_rays kind */
#define PT_RAY_HIT 1u          /* pt_RayHit::status bit 0: something was hit / the ray is occluded */
#define PT_RAY_INVALID 2u      /* bit 1: the ray was not walked (non-finite origin / direction, zero direction, NaN tmax of a bounded kind) */
#define PT_RAYS_DEVICE 1u      /* pt_trace_rays flags bit 0: rays and hits are device pointers on the context's GPU */
#define PT_RAYS_MAX_HITS 16u   /* largest hits_per_ray of PT_RAYS_CANDIDATES */
#define PT_QUERY_CHUNK (1u << 20) /* host arrays are staged through two device buffers of this many records (32 MB each) */

/* pt_trace_paths: one pt_Ray in, one record out (32 bytes, like pt_RayHit).  Stands in for what PathTrace of shaders/pathtrace.glsl returns along the
 * ray, averaged over the sample loop of shaders/pathtrace.comp; defined in DESIGN.md section 3.2 ("Path queries") and stated at pt_trace_paths. */
typedef struct pt_PathResult {
  float    radiance[3]; /* mean over the samples of the firefly-clamped path radiance */
  float    firstT;      /* t of the first sample's first closest hit; 0 on a miss */
  uint32_t seed;        /* RNG state after the last sample */
  uint32_t status;      /* PT_RAY_HIT: the first sample's first ray hit something; PT_RAY_INVALID: the ray was not walked */
  uint32_t closestRays; /* closest-hit rays traced over all samples */
  uint32_t _pad;        /* 0 */
} pt_PathResult;
#define PT_PATHS_MAX_SAMPLES 65536 /* largest RtxState.maxSamples of pt_trace_paths */

/* pt_gather: one point in, one record out -- the integral of the path loop's radiance over the directions that leave the point.  No reference
 * counterpart (the reference has no baker); each sample is PathTrace of shaders/pathtrace.glsl along a direction drawn at the point.  Defined in
 * DESIGN.md section 3.3 ("Gather queries") and stated at pt_gather. */
typedef struct pt_GatherPoint {
  float    position[3];
  uint32_t seed;      /* RNG state the point's samples start from */
  float    normal[3]; /* PT_GATHER_HEMISPHERE: any finite non-zero length fp32 can normalise (about 1e-19 .. 1.8e19: the squared length must neither
                       * underflow nor overflow); PT_GATHER_SPHERE: ignored, not even read for validity */
  uint32_t _pad;      /* ignored */
} pt_GatherPoint;
typedef struct pt_GatherResult { /* PT_GATHER_HEMISPHERE */
  float    irradiance[3]; /* pi x the mean over the cosine-distributed samples of the firefly-clamped path radiance */
  float    hitFraction;   /* samples whose first ray hit geometry / maxSamples */
  uint32_t seed;          /* RNG state after the last sample */
  uint32_t status;        /* 0 or PT_RAY_INVALID: the point was not walked */
  uint32_t closestRays;   /* closest-hit rays traced over all samples */
  uint32_t _pad;          /* 0 */
} pt_GatherResult;
typedef struct pt_ProbeResult { /* PT_GATHER_SPHERE */
  float    sh[9][3]; /* real spherical harmonics, bands 0 .. 2 in the order of DESIGN.md section 3.3, RGB per coefficient */
  float    hitFraction;
  uint32_t seed, status, closestRays, _pad; /* as in pt_GatherResult */
} pt_ProbeResult;
#define PT_GATHER_HEMISPHERE 0u /* pt_gather kind: cosine-distributed directions about the normal -> pt_GatherResult */
#define PT_GATHER_SPHERE 1u     /* uniform directions -> pt_ProbeResult */

/* pt_denoise / pt_tonemap_denoised: the edge-avoiding a-trous filter between the accumulation image and the display pass (no reference counterpart;
 * defined in DESIGN.md "Denoiser" and stated once in csrc/pt_denoise.h).  Guide planes are row-major RGBA32F images of the accumulation size whose
 * .xyz steer the weights; by convention plane 0 is the albedo (the only one PT_DENOISE_DEMODULATE reads), 1 the normal, 2 the depth in .x. */
#define PT_DENOISE_GUIDES 3
#define PT_DENOISE_DEMODULATE 1u /* pt_DenoiseParams::flags bit 0: filter colour / max(albedo, 0.001) and multiply the albedo back afterwards */
typedef struct pt_DenoiseParams {
  int32_t  iterations;                    /* 1 .. 8; iteration i taps at distance 2^i */
  float    sigmaColor;                    /* standard deviation of the colour term at iteration 0, halved every iteration; 0: no colour term */
  float    sigmaGuide[PT_DENOISE_GUIDES]; /* of the term of guide plane j; read only for the planes that are installed */
  uint32_t flags;                         /* PT_DENOISE_DEMODULATE */
} pt_DenoiseParams;

/* pt_temporal_accumulate: the temporal reprojection stage (no reference counterpart; defined in DESIGN.md section 5.3 and stated once in
 * csrc/pt_temporal.h).  pt_SceneCamera carries only inverses, so the caller supplies the forward matrix of the CURRENT camera (column-major, world ->
 * clip: proj * view; pt_camera_world_to_clip builds the one that belongs to pt_camera_lookat); the library keeps it with the history it writes. */
typedef struct pt_TemporalParams {
  float    worldToClip[16]; /* of the current camera; every entry finite */
  float    depthTol;        /* a history tap counts when |its depth - the expected depth| <= depthTol * the expected depth; > 0, finite */
  float    normalDist2;     /* ... and when the squared distance of the encoded normals is at most this ((1 - cos) / 2 for unit normals); >= 0, finite */
  float    maxHistory;      /* cap of the history length: the blend factor never falls below 1 / maxHistory; >= 1, finite */
  uint32_t flags;           /* none defined: must be 0 */
} pt_TemporalParams;

/* pt_temporal_fast: the responsive history (no reference counterpart; defined in DESIGN.md section 5.7 and stated once in csrc/pt_fast.h).  A second,
 * short history is kept beside the long one, and the long one is clamped to the short one's local mean +- sigmaScale standard deviations. */
typedef struct pt_FastParams {
  float    maxFast;    /* cap of the fast history's length, in the place of pt_TemporalParams::maxHistory; >= 1, finite (ReLAX: 4 .. 6) */
  float    sigmaScale; /* half width of the clamp interval in standard deviations of the fast history over the window; >= 0, finite */
  int32_t  radius;     /* the window is (2 radius + 1)^2 pixels; 1 .. 3 */
  uint32_t flags;      /* none defined: must be 0 */
} pt_FastParams;

/* pt_render_guides_chain: the guide pass that follows mirrors and clear glass to the first rough surface (no reference counterpart; defined in
 * DESIGN.md section 5.8 and stated once in csrc/pt_chain.h).  A surface is followed when its resolved roughness is at most maxRoughness and it is a
 * mirror (metallic >= minMetallic) or glass ((1 - metallic) * transmission >= minTransmission); a threshold above 1 turns that class off.  The
 * resolved roughness of a material is never below 0.001. */
#define PT_GUIDE_CHAIN_MAX_LINKS 8
typedef struct pt_GuideChain {
  uint32_t maxLinks;        /* 0 .. PT_GUIDE_CHAIN_MAX_LINKS: segments followed beyond the camera ray */
  float    maxRoughness;    /* a surface is followed only when its resolved roughness <= this; >= 0, finite */
  float    minMetallic;     /* mirror class:  metallic >= this; >= 0, finite */
  float    minTransmission; /* glass class:   (1 - metallic) * transmission >= this; >= 0, finite */
  uint32_t flags;           /* none defined; any bit is PT_ERR_INVALID */
} pt_GuideChain;

/* pt_svgf_variance / pt_svgf_history / pt_tonemap_svgf: the variance-guided filter of the history (no reference counterpart; defined in DESIGN.md
 * section 5.4 and stated once in csrc/pt_svgf.h).  The luminance edge stop is measured in standard deviations of the per-pixel variance estimate
 * that the moments in the history (pt_temporal_track_moments) give; guide terms are those of pt_DenoiseParams. */
typedef struct pt_SvgfParams {
  int32_t  iterations;                    /* 1 .. 8; iteration i taps at distance 2^i */
  float    sigmaLum;                      /* luminance differences are divided by sigmaLum * sqrt(variance) + lumFloor; > 0, finite (SVGF: 4) */
  float    lumFloor;                      /* > 0, finite: keeps the divisor positive where the variance is 0 */
  float    sigmaGuide[PT_DENOISE_GUIDES]; /* of the term of guide plane j; read only for the planes that are installed */
  float    minTemporal;                   /* a pixel whose history is shorter estimates its variance spatially; >= 1, finite (SVGF: 4) */
  uint32_t flags;                         /* none defined: must be 0 */
} pt_SvgfParams;

/* Counters the measurement contract needs; all totals since pt_reset_stats. */
typedef struct pt_Stats {
  uint64_t samples;          /* pixel-samples rendered */
  uint64_t closestRays;      /* rays through the closest-hit traversal kernel */
  uint64_t shadowRays;       /* rays through the shadow traversal */
  uint64_t shadedHits;       /* surface hits shaded */
  uint64_t misses;           /* environment lookups on miss */
  uint64_t alphaTests;       /* stochastic alpha evaluations */
  uint64_t neeLookups;       /* environment NEE samples */
  uint64_t nodesVisited;     /* BVH nodes popped (device layout; only in PT_STATS builds, else 0) */
  uint64_t trisTested;       /* triangle tests (only in PT_STATS builds, else 0) */
  double   msGenerate;       /* accumulated kernel time by stage, HIP events on the render stream */
  double   msTraceClosest;
  double   msShade;
  double   msTraceShadow;
  double   msAccumulate;
  uint64_t launchesTraceClosest;
  uint32_t numTriangles;     /* world-space triangles in the BVH */
  uint32_t numBvhNodes;
  double   msBuildAccel;     /* last pt_build_accel */
  uint64_t bytesScene;       /* resident HBM bytes of scene+BVH+textures+env */
  uint64_t bytesAccel;       /* of which the acceleration structure (nodes + leaf records + any-hit records) */
  uint32_t numBlas;          /* PT_ACCEL_TWO_LEVEL: bottom-level structures (prim-meshes instantiated), else 0 */
  uint32_t numTlasNodes;     /* PT_ACCEL_TWO_LEVEL: nodes of the instance hierarchy, else 0 */
  double   msTail;           /* kernel time of the fused late bounces (closest + shade + shadow of small queues in one launch) */
  uint32_t batchFrames;      /* frames traced as one wavefront after the path-state budget was applied (pt_resize) */
  uint32_t framesInFlight;   /* frame slots (a full batch each) overlapped on separate streams after the budget was applied; the one-frame display slots are not counted */
  uint64_t tailClosestRays;  /* the part of closestRays / shadowRays / shadedHits / misses / alphaTests that the fused late-bounce kernel processed */
  uint64_t tailShadowRays;
  uint64_t tailShadedHits;
  uint64_t tailMisses;
  uint64_t tailAlphaTests;
  uint64_t launchesTail;     /* launches of the fused late-bounce kernel (with profiling enabled, like launchesTraceClosest) */
  uint64_t numMergedTriangles; /* two-level mode: triangles of the prim-meshes instantiated once, kept in ONE world-space bottom-level structure
                                  (counted as one of numBlas); equal to numTriangles when the scene has no repeated mesh -- the flat kernels then run on it */
  double   msTraceFused;     /* kernel time of the fused trace stage: shadow rays of bounce b + closest-hit rays of bounce b + 1 in one launch
                                (msTraceClosest / msTraceShadow then hold bounce 0's closest-hit stage and the last staged bounce's shadow stage) */
  uint64_t launchesTraceFused;
} pt_Stats;

/* pt_refit_accel: what one refit did (no reference counterpart).  The tree cost is the sum over the used child boxes of every kept hierarchy -- the
 * flat one, or the merged world-space one and every BLAS -- of dx dy + dy dz + dz dx, taken in double from the fp32 planes.  costBefore belongs to
 * the structure as pt_build_accel left it (measured by the first refit after a build, before it changes a box, and kept); costAfter to the
 * structure this refit leaves.  costAfter / costBefore is what tells a caller when a rebuild is due.  (Two-level mode: when pt_update_instances moved a
 * once-instantiated node, the merged structure alone was built again; costBefore then holds its cost as just built plus the BLASes' as pt_build_accel left them.) */
typedef struct pt_RefitInfo {
  double   ms;           /* the call, by the host clock */
  double   costBefore;
  double   costAfter;
  uint32_t nodesWritten; /* 4-wide nodes whose boxes were made again */
  uint32_t slotsWritten; /* leaf slots whose records were made again */
} pt_RefitInfo;

/* pt_measure_peaks: ceilings measured on the device */
typedef struct pt_Peaks {
  double  valuWaveInstrPerSec; /* wave64 VALU instructions issued per second, whole chip */
  double  hbmCopyBytesPerSec;  /* read + written bytes per second of a streaming copy */
  double  hbmReadBytesPerSec;  /* bytes per second of a streaming read */
  int32_t computeUnits;
  int32_t clockMHz;
} pt_Peaks;

#ifdef __cplusplus
}
static_assert(sizeof(pt_RtxState) == 48, "RtxState");
static_assert(sizeof(pt_SceneCamera) == 140, "SceneCamera");
static_assert(sizeof(pt_VertexAttributes) == 32, "VertexAttributes");
static_assert(sizeof(pt_GltfShadeMaterial) == 216, "GltfShadeMaterial");
static_assert(sizeof(pt_Light) == 64, "Light");
static_assert(sizeof(pt_EnvAccel) == 16, "EnvAccel");
static_assert(sizeof(pt_Tonemapper) == 48, "Tonemapper");
static_assert(sizeof(pt_SunAndSky) == 96, "SunAndSky");
static_assert(sizeof(pt_PrimMesh) == 20, "PrimMesh");
static_assert(sizeof(pt_RefitInfo) == 32, "RefitInfo");
static_assert(sizeof(pt_Node) == 68, "Node");
static_assert(sizeof(pt_Ray) == 32 && sizeof(pt_RayHit) == 32, "Ray / RayHit");
static_assert(sizeof(pt_PathResult) == sizeof(pt_RayHit), "PathResult: staged through the buffers of pt_trace_rays");
static_assert(sizeof(pt_GatherPoint) == sizeof(pt_Ray) && sizeof(pt_GatherResult) == sizeof(pt_RayHit) && sizeof(pt_ProbeResult) == 4 * sizeof(pt_RayHit),
              "GatherPoint / GatherResult / ProbeResult: staged through the buffers of pt_trace_rays");
static_assert(sizeof(pt_DenoiseParams) == 24, "DenoiseParams");
static_assert(sizeof(pt_TemporalParams) == 80, "TemporalParams");
static_assert(sizeof(pt_SvgfParams) == 32, "SvgfParams");
static_assert(sizeof(pt_FastParams) == 16, "FastParams");
static_assert(sizeof(pt_GuideChain) == 20, "GuideChain");
#endif

#endif /* PT_TYPES_H */
