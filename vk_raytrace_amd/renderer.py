"""Host-side mirror of the reference's renderer interface for the gfx950 backend.

``Renderer`` has the reference's method set and call order (reference: src/renderer.h:30-48);
``HipRenderer`` is the implementation that takes the place of ``RayQuery`` (src/rayquery.cpp:40-109)
and ``RtxPipeline`` (src/rtx_pipeline.cpp:45-276).  ``SampleExample`` is the headless part of the
reference's orchestrator that the hot path needs (src/sample_example.cpp:77-82 setup loop,
:90-111 load, :183-207 frame counter, :322-337 createRender, :390-429 renderScene, :362-384 drawPost).

Vulkan handles do not exist on the target: what reached the shaders through descriptor sets
(TLAS, output image, scene buffers, environment) is handed over with explicit ``set_*`` calls, and
the command buffer is the context's own HIP stream.
"""
import ctypes as C
import os

import numpy as np

from . import capi
from . import host_device as hd


class Renderer:
    """reference: src/renderer.h:30-48"""

    def __init__(self):
        self.m_state = hd.RtxState()

    def setup(self, device, physicalDevice=None, familyIndex=0, allocator=None):
        raise NotImplementedError

    def destroy(self):
        raise NotImplementedError

    def run(self, cmdBuf, size, profiler, extraDescSets):
        raise NotImplementedError

    def create(self, size, extraDescSetsLayout, scene=None):
        raise NotImplementedError

    def name(self):
        raise NotImplementedError

    def setPushContants(self, state):  # (sic) the reference's spelling, src/renderer.h:44
        self.m_state = state


def pixel_centre_rays(cam: hd.SceneCamera, width, height):
    """The pinhole camera rays through the pixel centres, built the way pt_pick builds its ray from a window position:
    origin = viewInverse * (0, 0, 0, 1), direction = viewInverse * (normalize((projInverse * (d, 1, 1)).xyz), 0) with d = 2 * (pixel + 0.5) / size - 1.
    Returns (origins, directions), float32 arrays of shape (height * width, 3) in row-major pixel order."""
    vi = np.array(cam.viewInverse, np.float64).reshape(4, 4).T  # column-major storage
    pi = np.array(cam.projInverse, np.float64).reshape(4, 4).T
    ys, xs = np.mgrid[0:height, 0:width]
    d = np.stack([2 * (xs + 0.5) / width - 1, 2 * (ys + 0.5) / height - 1, np.ones(xs.shape), np.ones(xs.shape)], -1).reshape(-1, 4)
    target = d @ pi.T
    t3 = target[:, :3] / np.linalg.norm(target[:, :3], axis=1, keepdims=True)
    directions = t3 @ vi[:3, :3].T
    origins = np.broadcast_to(vi[:3, 3], directions.shape)
    return np.ascontiguousarray(origins, np.float32), np.ascontiguousarray(directions, np.float32)


class HipRenderer(Renderer):
    """libptmi.so behind the reference's Renderer interface."""

    def __init__(self):
        super().__init__()
        self._lib = capi.lib()
        self._ctx = None
        self._display_sizes = []  # viewports of the images begun with tonemap_begin and not collected yet
        self._keep = None
        self._camera = None
        self.size = (0, 0)
        self.env_integral = 1.0
        self.env_average = 1.0

    # -- Renderer interface ------------------------------------------------------------------------
    def setup(self, device=0, physicalDevice=None, familyIndex=0, allocator=None):
        """Renderer::setup: bind to one GPU (`device` is the HIP ordinal)."""
        if self._ctx is not None:
            return
        self._display_sizes = []  # a new context has no display image pending
        ctx = C.c_void_p()
        rc = self._lib.pt_create(int(device), C.byref(ctx))
        if rc != capi.PT_OK:
            raise capi.PtError(rc, self._lib.pt_last_error(None).decode())
        self._ctx = ctx

    def destroy(self):
        if self._ctx is not None:
            self._lib.pt_destroy(self._ctx)
            self._ctx = None
        self._display_sizes = []  # the C side's display ring went with the context

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def name(self):
        return self._lib.pt_renderer_name().decode()

    def create(self, size, extraDescSetsLayout=None, scene=None):
        """Renderer::create(size, layouts, scene): allocate the output for `size` = (width, height);
        if a scene is given it is uploaded and its acceleration structure built."""
        if scene is not None:
            self.set_scene(scene)
        self._check(self._lib.pt_resize(self._ctx, int(size[0]), int(size[1])))
        self.size = (int(size[0]), int(size[1]))

    def run(self, cmdBuf=None, size=None, profiler=None, extraDescSets=None):
        """Renderer::run: one frame with the state given to setPushContants (asynchronous)."""
        if size is not None and tuple(size) != self.size:
            self.create(size)
        self.m_state.size[0], self.m_state.size[1] = self.size
        self._check(self._lib.pt_render_frame(self._ctx, C.byref(self.m_state)))

    # -- what the descriptor sets carried -------------------------------------------------------------
    def set_scene(self, scene):
        d, keep = scene.desc()
        self._check(self._lib.pt_set_scene(self._ctx, C.byref(d)))
        self._check(self._lib.pt_build_accel(self._ctx))
        self._keep = keep

    def set_env(self, env_rgba32f):
        env = np.ascontiguousarray(env_rgba32f, np.float32)
        assert env.ndim == 3 and env.shape[2] == 4
        i, a = C.c_float(), C.c_float()
        self._check(self._lib.pt_set_env(self._ctx, env.ctypes.data, env.shape[1], env.shape[0], C.byref(i), C.byref(a)))
        self.env_integral, self.env_average = i.value, a.value
        return self.env_integral, self.env_average

    def set_camera(self, cam: hd.SceneCamera):
        self._check(self._lib.pt_set_camera(self._ctx, C.byref(cam)))
        self._camera = hd.SceneCamera.from_buffer_copy(cam)  # render_guides shoots its depth rays through it

    def set_sunsky(self, ss: hd.SunAndSky):
        self._check(self._lib.pt_set_sunsky(self._ctx, C.byref(ss)))

    def useAnyHit(self, enable):
        """RtxPipeline::useAnyHit (src/rtx_pipeline.cpp:269-276)"""
        self._check(self._lib.pt_use_any_hit(self._ctx, int(bool(enable))))

    def set_accel_mode(self, mode):
        """capi.PT_ACCEL_FLAT (default: one hierarchy over all world-space triangles) or capi.PT_ACCEL_TWO_LEVEL (the reference's
        BLAS per prim-mesh + TLAS instance per node, src/accelstruct.cpp:110-162)."""
        self._check(self._lib.pt_set_accel_mode(self._ctx, int(mode)))

    def update_instances(self, nodes):
        """New world matrices for the scene's nodes (hd.node_dtype array or scene.Scene): TLAS refit in two-level mode, rebuild otherwise."""
        arr = np.ascontiguousarray(nodes.node_array() if hasattr(nodes, "node_array") else nodes, hd.node_dtype)
        self._check(self._lib.pt_update_instances(self._ctx, arr.ctypes.data, len(arr)))

    def update_vertices(self, first, vertices):
        """Replaces vertices[first : first + len(vertices)] of the scene's vertex buffer (whole records of capi.pack_vertices' dtype).  A built
        structure is stale afterwards: refit_accel() or build_accel() before anything walks it."""
        arr = np.ascontiguousarray(vertices)
        assert arr.dtype.itemsize == C.sizeof(hd.VertexAttributes), "vertices: records of 32 bytes (capi.pack_vertices)"
        self._check(self._lib.pt_update_vertices(self._ctx, int(first), len(arr), arr.ctypes.data if len(arr) else None))

    def refit_accel(self):
        """Brings the stale structure up to date without changing its topology -> hd.RefitInfo (costAfter / costBefore says when to rebuild)."""
        info = hd.RefitInfo()
        self._check(self._lib.pt_refit_accel(self._ctx, C.byref(info)))
        return info

    def set_variant(self, variant):
        """capi.PT_VARIANT_RAYQUERY (the reference's RayQuery renderer, default) or capi.PT_VARIANT_RTX (its RtxPipeline)."""
        self._check(self._lib.pt_set_variant(self._ctx, int(variant)))

    def set_shard(self, rank, nranks):
        self._check(self._lib.pt_set_shard(self._ctx, rank, nranks))

    # -- output --------------------------------------------------------------------------------------
    def synchronize(self):
        self._check(self._lib.pt_synchronize(self._ctx))

    def read_accum(self):
        w, h = self.size
        out = np.empty((h, w, 4), np.float32)
        self._check(self._lib.pt_read_accum(self._ctx, out.ctypes.data))
        return out

    def write_accum(self, img):
        """Checkpoint restore: replaces the accumulation image (continue with RtxState.frame = frames already in it)."""
        w, h = self.size
        img = np.ascontiguousarray(img, np.float32)
        assert img.shape == (h, w, 4)
        self._check(self._lib.pt_write_accum(self._ctx, img.ctypes.data))

    def pick(self, x, y, cam: hd.SceneCamera):
        """SampleExample::screenPicking (src/sample_example.cpp:468-511): nearest triangle under the normalised window position."""
        out = hd.PickResult()
        vi = (C.c_float * 16)(*cam.viewInverse)
        pi = (C.c_float * 16)(*cam.projInverse)
        self._check(self._lib.pt_pick(self._ctx, float(x), float(y), vi, pi, C.byref(out)))
        return out

    def trace_rays(self, kind, origins, directions, tmax=None, seeds=None, hits_per_ray=1):
        """pt_trace_rays on host arrays: `kind` is capi.PT_RAYS_CLOSEST / OCCLUDED / NEAREST / CANDIDATES; origins, directions: (n, 3); tmax (scalar
        or (n,), default +inf: unbounded) bounds every kind but CLOSEST; seeds (n,) uint32 (default 0) feed the alpha draws.  Returns a structured
        array (hd.rayhit_dtype) of shape (n,), or (n, hits_per_ray) for CANDIDATES."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError("trace_rays: origins and directions differ in length")
        rays = np.zeros(len(o), hd.ray_dtype)
        rays["origin"], rays["direction"] = o, d
        rays["tmax"] = np.inf if tmax is None else np.asarray(tmax, np.float32)
        rays["seed"] = 0 if seeds is None else np.asarray(seeds, np.uint32)
        return self.trace_ray_records(kind, rays, hits_per_ray)

    def trace_ray_records(self, kind, rays, hits_per_ray=1):
        """pt_trace_rays on an array of hd.ray_dtype records (what trace_rays assembles)"""
        rays = np.ascontiguousarray(rays, hd.ray_dtype)
        hits = np.zeros((len(rays), int(hits_per_ray)), hd.rayhit_dtype)
        self._check(self._lib.pt_trace_rays(self._ctx, int(kind), 0, len(rays), rays.ctypes.data, hits.ctypes.data, int(hits_per_ray)))
        return hits if int(kind) == capi.PT_RAYS_CANDIDATES else hits[:, 0]

    def trace_rays_device(self, kind, rays_ptr, hits_ptr, n, hits_per_ray=1):
        """pt_trace_rays with PT_RAYS_DEVICE: rays_ptr / hits_ptr are plain integers, the addresses of n pt_Ray and n * hits_per_ray pt_RayHit records
        in the memory of the context's GPU (16-byte aligned), e.g. a torch tensor's data_ptr().  The caller owns the memory and keeps it alive;
        the results are in place when the call returns."""
        self._check(self._lib.pt_trace_rays(self._ctx, int(kind), capi.PT_RAYS_DEVICE, int(n), C.c_void_p(int(rays_ptr)), C.c_void_p(int(hits_ptr)), int(hits_per_ray)))

    def trace_paths(self, state: hd.RtxState, origins, directions, seeds=None):
        """pt_trace_paths on host arrays: the radiance along each ray (origins, directions: (n, 3); seeds (n,) uint32, default 0: the RNG state each
        ray's paths start from) under `state` -- maxDepth, maxSamples, fireflyClampThreshold, hdrMultiplier, pbrMode and debugging_mode are read.
        Returns a structured array (hd.pathresult_dtype) of shape (n,)."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError("trace_paths: origins and directions differ in length")
        rays = np.zeros(len(o), hd.ray_dtype)
        rays["origin"], rays["direction"] = o, d
        rays["tmax"] = np.inf  # (ignored: the first ray of a path is unbounded)
        rays["seed"] = 0 if seeds is None else np.asarray(seeds, np.uint32)
        return self.trace_path_records(state, rays)

    def trace_path_records(self, state: hd.RtxState, rays):
        """pt_trace_paths on an array of hd.ray_dtype records (what trace_paths assembles)"""
        rays = np.ascontiguousarray(rays, hd.ray_dtype)
        out = np.zeros(len(rays), hd.pathresult_dtype)
        self._check(self._lib.pt_trace_paths(self._ctx, C.byref(state), 0, len(rays), rays.ctypes.data, out.ctypes.data))
        return out

    def trace_paths_device(self, state: hd.RtxState, rays_ptr, results_ptr, n):
        """pt_trace_paths with PT_RAYS_DEVICE: rays_ptr / results_ptr are plain integers, the addresses of n pt_Ray and n pt_PathResult records in the
        memory of the context's GPU (16-byte aligned), e.g. a torch tensor's data_ptr().  The caller owns the memory and keeps it alive; the results
        are in place when the call returns."""
        self._check(self._lib.pt_trace_paths(self._ctx, C.byref(state), capi.PT_RAYS_DEVICE, int(n), C.c_void_p(int(rays_ptr)), C.c_void_p(int(results_ptr))))

    def gather_irradiance(self, state: hd.RtxState, positions, normals, seeds=None):
        """pt_gather, PT_GATHER_HEMISPHERE, on host arrays: the irradiance at each point (positions, normals: (n, 3), normals of any non-zero length;
        seeds (n,) uint32, default 0: the RNG state each point's samples start from) from state.maxSamples cosine-distributed paths under `state`
        (the fields pt_trace_paths reads).  Returns a structured array (hd.gatherresult_dtype) of shape (n,)."""
        return self.gather_records(state, capi.PT_GATHER_HEMISPHERE, self._gather_points("gather_irradiance", positions, normals, seeds))

    def gather_probes(self, state: hd.RtxState, positions, seeds=None):
        """pt_gather, PT_GATHER_SPHERE, on host arrays: nine spherical-harmonic coefficients (bands 0 .. 2, RGB) of the radiance arriving at each
        position from state.maxSamples uniformly distributed paths.  Returns a structured array (hd.proberesult_dtype) of shape (n,)."""
        return self.gather_records(state, capi.PT_GATHER_SPHERE, self._gather_points("gather_probes", positions, None, seeds))

    @staticmethod
    def _gather_points(who, positions, normals, seeds):
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        pts = np.zeros(len(p), hd.gatherpoint_dtype)
        pts["position"] = p
        if normals is not None:
            nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
            if len(nrm) != len(p):
                raise ValueError(f"{who}: positions and normals differ in length")
            pts["normal"] = nrm
        pts["seed"] = 0 if seeds is None else np.asarray(seeds, np.uint32)
        return pts

    def gather_records(self, state: hd.RtxState, kind, points):
        """pt_gather on an array of hd.gatherpoint_dtype records (what gather_irradiance / gather_probes assemble): hd.gatherresult_dtype records for
        capi.PT_GATHER_HEMISPHERE, hd.proberesult_dtype records for capi.PT_GATHER_SPHERE"""
        points = np.ascontiguousarray(points, hd.gatherpoint_dtype)
        out = np.zeros(len(points), hd.proberesult_dtype if int(kind) == capi.PT_GATHER_SPHERE else hd.gatherresult_dtype)
        self._check(self._lib.pt_gather(self._ctx, C.byref(state), int(kind), 0, len(points), points.ctypes.data, out.ctypes.data))
        return out

    def gather_device(self, state: hd.RtxState, kind, points_ptr, results_ptr, n):
        """pt_gather with PT_RAYS_DEVICE: points_ptr / results_ptr are plain integers, the addresses of n pt_GatherPoint records and n records of the
        kind's result type in the memory of the context's GPU (16-byte aligned), e.g. a torch tensor's data_ptr().  The caller owns the memory and
        keeps it alive; the results are in place when the call returns."""
        self._check(self._lib.pt_gather(self._ctx, C.byref(state), int(kind), capi.PT_RAYS_DEVICE, int(n), C.c_void_p(int(points_ptr)), C.c_void_p(int(results_ptr))))

    def tonemap(self, tm: hd.Tonemapper, display_size=None):
        """RenderOutput::genMipmap + run.  display_size (W, H): the viewport while de-scaling (Tonemapper.zoom = 1 / level)."""
        w, h = display_size or self.size
        out = np.empty((h, w, 4), np.uint8)
        if display_size is None:
            self._check(self._lib.pt_tonemap(self._ctx, C.byref(tm), out.ctypes.data))
        else:
            self._check(self._lib.pt_tonemap_zoom(self._ctx, C.byref(tm), w, h, out.ctypes.data))
        return out

    # -- denoiser (no reference counterpart) ----------------------------------------------------------
    def set_denoise_guides(self, albedo=None, normal=None, depth=None):
        """pt_set_denoise_guides: each plane is None (unset) or an (H, W, 4) float32 image whose .xyz steer the filter's weights"""
        w, h = self.size
        planes = [None if p is None else np.ascontiguousarray(p, np.float32) for p in (albedo, normal, depth)]
        for p in planes:
            if p is not None and p.shape != (h, w, 4):
                raise ValueError(f"set_denoise_guides: a plane of shape {p.shape}, the image is {(h, w, 4)}")
        ptrs = (C.c_void_p * capi.PT_DENOISE_GUIDES)(*[None if p is None else p.ctypes.data for p in planes])
        self._check(self._lib.pt_set_denoise_guides(self._ctx, ptrs))

    def denoise(self, params: hd.DenoiseParams):
        """pt_denoise: the image read_accum() would return, filtered ((H, W, 4) float32)"""
        w, h = self.size
        out = np.empty((h, w, 4), np.float32)
        self._check(self._lib.pt_denoise(self._ctx, C.byref(params), out.ctypes.data))
        return out

    def tonemap_denoised(self, params: hd.DenoiseParams, tm: hd.Tonemapper):
        """pt_tonemap_denoised: tonemap() of the denoised image"""
        w, h = self.size
        out = np.empty((h, w, 4), np.uint8)
        self._check(self._lib.pt_tonemap_denoised(self._ctx, C.byref(params), C.byref(tm), out.ctypes.data))
        return out

    def render_guides(self, state: hd.RtxState, miss_depth=1.0e30):
        """Guide planes for the current camera, from entry points that exist for other purposes: one frame-0 debug frame each for base colour and
        normal, and the closest-hit distance of the pixel-centre camera rays (`t` in .x; `miss_depth` where nothing is hit).  Installs all three
        and returns them.  To be called right after a camera change, before frame 0 of the real accumulation: frame 0 overwrites the accumulation
        image, so nothing needs saving.  `state`: the push constants of the frames to come (not modified); the camera is what set_camera was given.
        capture_guides renders the same planes on the device in one pass, without a frame and without a copy."""
        if self._camera is None:
            raise capi.PtError(capi.PT_ERR_STATE, "render_guides before set_camera")
        w, h = self.size
        st = hd.RtxState.from_buffer_copy(state)
        st.frame, st.size[0], st.size[1] = 0, w, h
        planes = []
        for mode in (hd.eBaseColor, hd.eNormal):
            st.debugging_mode = mode
            self._check(self._lib.pt_render_frame(self._ctx, C.byref(st)))
            planes.append(self.read_accum())
        origins, directions = pixel_centre_rays(self._camera, w, h)
        hits = self.trace_rays(capi.PT_RAYS_CLOSEST, origins, directions)
        depth = np.zeros((h, w, 4), np.float32)
        depth[..., 0] = np.where(hits["status"] & capi.PT_RAY_HIT, hits["t"], np.float32(miss_depth)).reshape(h, w)
        planes.append(depth)
        self.set_denoise_guides(*planes)
        return tuple(planes)

    def capture_guides(self, planes=7, miss_depth=1.0e30):
        """pt_render_guides: the guide planes selected by `planes` (capi.PT_GUIDES_BASECOLOR | PT_GUIDES_NORMAL | PT_GUIDES_DEPTH) for the current
        camera, rendered on the device into the context's guide planes by one first-hit pass.  Asynchronous like run(); a plane outside the mask
        stays as it is.  The depth plane holds `miss_depth` where nothing is hit."""
        self._check(self._lib.pt_render_guides(self._ctx, int(planes), float(miss_depth)))

    @staticmethod
    def guide_chain(max_links=4, max_roughness=0.05, min_metallic=0.9, min_transmission=0.9):
        """an hd.GuideChain: follow at most max_links segments through surfaces of resolved roughness <= max_roughness that are mirrors (metallic >=
        min_metallic) or clear glass ((1 - metallic) * transmission >= min_transmission); a threshold above 1 turns that class off"""
        return hd.GuideChain(maxLinks=max_links, maxRoughness=max_roughness, minMetallic=min_metallic, minTransmission=min_transmission, flags=0)

    def capture_guides_chain(self, chain, planes=7, miss_depth=1.0e30):
        """pt_render_guides_chain: capture_guides for the first surface behind mirrors and clear glass: plane 0 the product of
        the base colours along the chain, plane 1 the end surface's normal, plane 2 the summed length.  Asynchronous; read_guides returns the planes,
        read_guide_chain the link plane."""
        self._check(self._lib.pt_render_guides_chain(self._ctx, C.byref(chain), int(planes), float(miss_depth)))

    def read_guide_chain(self):
        """pt_read_guide_chain: the link plane of the latest capture_guides_chain, (H, W) uint32: links | end << 8 (end: 0 a surface that is not
        followed, 1 a miss, 2 the link limit, 3 a direction that cannot be followed)"""
        w, h = self.size
        out = np.empty((h, w), np.uint32)
        self._check(self._lib.pt_read_guide_chain(self._ctx, out.ctypes.data))
        return out

    def read_guides(self, planes=None):
        """pt_read_denoise_guides: the installed guide planes as a tuple of three (H, W, 4) float32 images.  planes: mask of the planes to read
        (None: all three); a plane outside it comes back as None, one inside it that is not installed is an error (PT_ERR_STATE)."""
        w, h = self.size
        mask = 7 if planes is None else int(planes)
        out = [np.empty((h, w, 4), np.float32) if mask & (1 << j) else None for j in range(capi.PT_DENOISE_GUIDES)]
        ptrs = (C.c_void_p * capi.PT_DENOISE_GUIDES)(*[None if p is None else p.ctypes.data for p in out])
        self._check(self._lib.pt_read_denoise_guides(self._ctx, ptrs))
        return tuple(out)

    # -- temporal reprojection (no reference counterpart) ----------------------------------------------
    @staticmethod
    def world_to_clip(camera, aspect):
        """The forward matrix (proj * view, column-major, 16 float32) of a scene.Camera at `aspect`: TemporalParams.worldToClip of the camera that
        set_camera was given (pt_camera_world_to_clip)"""
        return capi.camera_world_to_clip(camera, aspect)

    @staticmethod
    def temporal_params(world_to_clip, depth_tol=0.05, normal_dist2=0.05, max_history=32.0):
        return hd.TemporalParams(worldToClip=tuple(float(v) for v in np.asarray(world_to_clip, np.float32).reshape(16)), depthTol=depth_tol,
                                 normalDist2=normal_dist2, maxHistory=max_history, flags=0)

    def temporal_accumulate(self, params: hd.TemporalParams, read=True):
        """pt_temporal_accumulate: reprojects the history into the current camera and blends the accumulation image into it; needs guide planes 1
        and 2 (capture_guides).  Returns the new history colour ((H, W, 4) float32), or None with read=False."""
        w, h = self.size
        out = np.empty((h, w, 4), np.float32) if read else None
        self._check(self._lib.pt_temporal_accumulate(self._ctx, C.byref(params), None if out is None else out.ctypes.data))
        return out

    def temporal_reset(self):
        """pt_temporal_reset: drops the history (scene change, cut)"""
        self._check(self._lib.pt_temporal_reset(self._ctx))

    def read_temporal_history(self):
        """pt_read_temporal_history: (colour (H, W, 4), length (H, W)) float32"""
        w, h = self.size
        colour, length = np.empty((h, w, 4), np.float32), np.empty((h, w), np.float32)
        self._check(self._lib.pt_read_temporal_history(self._ctx, colour.ctypes.data, length.ctypes.data))
        return colour, length

    def denoise_history(self, params: hd.DenoiseParams):
        """pt_denoise_history: denoise() of the history's colour image"""
        w, h = self.size
        out = np.empty((h, w, 4), np.float32)
        self._check(self._lib.pt_denoise_history(self._ctx, C.byref(params), out.ctypes.data))
        return out

    def tonemap_history(self, params, tm: hd.Tonemapper):
        """pt_tonemap_history: tonemap() of the history's colour image, spatially filtered first unless params is None"""
        w, h = self.size
        out = np.empty((h, w, 4), np.uint8)
        self._check(self._lib.pt_tonemap_history(self._ctx, None if params is None else C.byref(params), C.byref(tm), out.ctypes.data))
        return out

    # -- motion of moving instances (no reference counterpart) -----------------------------------------
    def render_instance_plane(self, guide_planes=7, miss_depth=1.0e30):
        """pt_render_instance_plane: capture_guides(guide_planes, miss_depth) -- the mask may be 0 here -- with the instance plane written besides by
        the same first-hit pass: per pixel the node index of the hit, capi.PT_INSTANCE_NONE for a miss.  Asynchronous like run()."""
        self._check(self._lib.pt_render_instance_plane(self._ctx, int(guide_planes), float(miss_depth)))

    def set_instance_plane(self, ids):
        """pt_set_instance_plane: an (H, W) uint32 plane of node indices (any other word: no instance), or None to drop the plane"""
        if ids is None:
            self._check(self._lib.pt_set_instance_plane(self._ctx, None))
            return
        w, h = self.size
        ids = np.ascontiguousarray(ids, np.uint32)
        if ids.shape != (h, w):
            raise ValueError(f"set_instance_plane: a plane of shape {ids.shape}, the image is {(h, w)}")
        self._check(self._lib.pt_set_instance_plane(self._ctx, ids.ctypes.data))

    def read_instance_plane(self):
        """pt_read_instance_plane: the installed instance plane, (H, W) uint32"""
        w, h = self.size
        out = np.empty((h, w), np.uint32)
        self._check(self._lib.pt_read_instance_plane(self._ctx, out.ctypes.data))
        return out

    def temporal_accumulate_moving(self, params: hd.TemporalParams, read=True):
        """pt_temporal_accumulate_moving: temporal_accumulate() for a scene whose nodes moved since the history was made (update_instances); pixels of
        a moved node take their point and normal through its motion before they are reprojected.  Needs the instance plane besides guide planes 1
        and 2 (render_instance_plane).  Returns the new history colour ((H, W, 4) float32), or None with read=False."""
        w, h = self.size
        out = np.empty((h, w, 4), np.float32) if read else None
        self._check(self._lib.pt_temporal_accumulate_moving(self._ctx, C.byref(params), None if out is None else out.ctypes.data))
        return out

    # -- demodulated history (no reference counterpart) ------------------------------------------------
    def temporal_demodulate(self, on=True):
        """pt_temporal_demodulate: the temporal step divides the pixel's own colour by guide plane 0 (the albedo) as it reads it, so that the history,
        its moments and the filters work on illumination, and svgf_history / tonemap_svgf / denoise_history / tonemap_history multiply their final
        image by guide plane 0 again.  temporal_accumulate[_moving] and read_temporal_history return illumination then.  A change drops the history."""
        self._check(self._lib.pt_temporal_demodulate(self._ctx, int(on)))

    # -- responsive history (no reference counterpart) --------------------------------------------------
    @staticmethod
    def fast_params(max_fast=4.0, sigma_scale=2.0, radius=2):
        return hd.FastParams(maxFast=max_fast, sigmaScale=sigma_scale, radius=radius, flags=0)

    def temporal_fast(self, params):
        """pt_temporal_fast: with an hd.FastParams, temporal_accumulate[_moving] keep a second, short history (maxFast in the place of maxHistory) beside
        the long one, clamp the long one to the short one's mean +- sigmaScale standard deviations over a (2 radius + 1)^2 window and cut the history
        length to maxFast where the clamp moved a channel: lighting changes the guides cannot see show within a few frames.  None: off.  Going from
        off to on or back drops the history; new parameters do not."""
        self._check(self._lib.pt_temporal_fast(self._ctx, None if params is None else C.byref(params)))

    def read_temporal_fast(self):
        """pt_read_temporal_fast: the fast history, (colour (H, W, 4), length (H, W)) float32"""
        w, h = self.size
        colour, length = np.empty((h, w, 4), np.float32), np.empty((h, w), np.float32)
        self._check(self._lib.pt_read_temporal_fast(self._ctx, colour.ctypes.data, length.ctypes.data))
        return colour, length

    # -- variance-guided filter of the history (no reference counterpart) ------------------------------
    @staticmethod
    def svgf_params(iterations=5, sigma_lum=4.0, lum_floor=1.0e-4, sigma_guide=(1.0, 0.3, 0.5), min_temporal=4.0):
        return hd.SvgfParams(iterations=iterations, sigmaLum=sigma_lum, lumFloor=lum_floor, sigmaGuide=tuple(float(v) for v in sigma_guide),
                             minTemporal=min_temporal, flags=0)

    def track_moments(self, on=True):
        """pt_temporal_track_moments: the history also keeps the first two moments of the luminance; a change drops the history"""
        self._check(self._lib.pt_temporal_track_moments(self._ctx, int(on)))

    def read_temporal_moments(self):
        """pt_read_temporal_moments: (H, W, 2) float32, (m1, m2)"""
        w, h = self.size
        out = np.empty((h, w, 2), np.float32)
        self._check(self._lib.pt_read_temporal_moments(self._ctx, out.ctypes.data))
        return out

    def svgf_variance(self, params: hd.SvgfParams):
        """pt_svgf_variance: the initial variance estimate of the history ((H, W) float32)"""
        w, h = self.size
        out = np.empty((h, w), np.float32)
        self._check(self._lib.pt_svgf_variance(self._ctx, C.byref(params), out.ctypes.data))
        return out

    def svgf_history(self, params: hd.SvgfParams, variance=True):
        """pt_svgf_history: (the filtered history (H, W, 4), the variance after the last iteration (H, W) or None with variance=False), float32"""
        w, h = self.size
        out = np.empty((h, w, 4), np.float32)
        var = np.empty((h, w), np.float32) if variance else None
        self._check(self._lib.pt_svgf_history(self._ctx, C.byref(params), out.ctypes.data, None if var is None else var.ctypes.data))
        return out, var

    def tonemap_svgf(self, params: hd.SvgfParams, tm: hd.Tonemapper):
        """pt_tonemap_svgf: tonemap() of svgf_history()'s image"""
        w, h = self.size
        out = np.empty((h, w, 4), np.uint8)
        self._check(self._lib.pt_tonemap_svgf(self._ctx, C.byref(params), C.byref(tm), out.ctypes.data))
        return out

    def tonemap_begin(self, tm: hd.Tonemapper, display_size=None):
        """pt_tonemap_begin: the display pass enqueued behind the frames rendered so far; later frames overlap it.  tonemap_end() returns the
        oldest image begun (at most 4 may be pending)."""
        w, h = display_size or self.size
        self._check(self._lib.pt_tonemap_begin(self._ctx, C.byref(tm), w, h))  # raises before the shadow list grows: the two stay in step
        self._display_sizes.append((w, h))

    def tonemap_pending(self):
        return int(self._lib.pt_tonemap_pending(self._ctx))

    def tonemap_end(self):
        if not self._display_sizes:
            self._check(self._lib.pt_tonemap_end(self._ctx, np.empty(4, np.uint8).ctypes.data))  # reports the error
        if self.tonemap_pending() != len(self._display_sizes):  # the C side is the truth; never size a buffer from a stale shadow entry
            self._display_sizes = []
            raise capi.PtError(capi.PT_ERR_STATE, "tonemap_end: the display ring and its Python shadow disagree (context re-created?)")
        w, h = self._display_sizes[0]
        out = np.empty((h, w, 4), np.uint8)
        pending = self.tonemap_pending()
        rc = self._lib.pt_tonemap_end(self._ctx, out.ctypes.data)
        if self.tonemap_pending() < pending:  # collected, also when it reports an error (a traversal-stack overflow): the two stay in step
            self._display_sizes.pop(0)
        self._check(rc)
        return out

    def measure_peaks(self):
        """pt_measure_peaks: VALU issue and HBM streaming ceilings measured on this device (dict)"""
        p = hd.Peaks()
        self._check(self._lib.pt_measure_peaks(self._ctx, C.byref(p)))
        return {k: getattr(p, k) for k, _ in hd.Peaks._fields_}

    def local_shard(self):
        ptr, nbytes, nloc, nmax = C.c_void_p(), C.c_size_t(), C.c_int(), C.c_int()
        self._check(self._lib.pt_local_shard(self._ctx, C.byref(ptr), C.byref(nbytes), C.byref(nloc), C.byref(nmax)))
        return ptr.value, nbytes.value, nloc.value, nmax.value

    def scatter_shards(self, gathered_device_ptr, nranks):
        self._check(self._lib.pt_scatter_shards(self._ctx, C.c_void_p(gathered_device_ptr), nranks))

    # -- measurement -----------------------------------------------------------------------------------
    def set_profiling(self, enable):
        self._check(self._lib.pt_set_profiling(self._ctx, int(enable)))

    def stats(self):
        s = hd.Stats()
        self._check(self._lib.pt_get_stats(self._ctx, C.byref(s)))
        return s.as_dict()

    def reset_stats(self):
        self._check(self._lib.pt_reset_stats(self._ctx))

    def _check(self, rc):
        if rc != capi.PT_OK:
            raise capi.PtError(rc, self._lib.pt_last_error(self._ctx).decode())


class SampleExample:
    """The headless slice of the reference's orchestrator (src/sample_example.{hpp,cpp}): scene / environment loading, the frame counter with its
    camera-change detection, the de-scaling state machine of the mouse callbacks, renderScene and drawPost."""

    def __init__(self, device=0, renderer=None):
        self.m_rtxState = hd.default_rtx_state()       # sample_example.hpp:162-174
        self.m_sunAndSky = hd.default_sun_and_sky()    # sample_example.hpp:176-193
        self.m_tonemapper = hd.default_tonemapper()    # render_output.hpp:37-49
        self.m_maxFrames = 100000                      # sample_example.hpp:195
        self.m_descaling = False                       # sample_example.hpp:197
        self.m_descalingLevel = 1                      # sample_example.hpp:198
        self.m_framesInFlight = 0                      # display images the host lets the GPU run behind (drawPost); the reference's swapchain ring
        self.m_pRender = renderer if renderer is not None else HipRenderer()
        self.m_pRender.setup(device)                   # sample_example.cpp:77-82
        self.m_scene = None
        self.m_size = (0, 0)                           # m_renderRegion.extent
        self._refCamMatrix = None                      # updateFrame's `static glm::mat4 refCamMatrix` / `static float fov`
        self._refFov = 0.0
        self._inputs = {"lmb": False, "mmb": False, "rmb": False}  # AppBaseVk::m_inputs
        self.resetFrame()

    # sample_example.cpp:90-98 loadScene + main.cpp:186-189.  A path goes through libptmi's own importer (pt_gltf_load), like Scene::load.
    def loadScene(self, scene):
        if isinstance(scene, (str, bytes, os.PathLike)):
            from .scene import GltfFileScene
            scene = GltfFileScene(os.fsdecode(scene))
        if scene.vertices is None:
            scene.finalize(capi.pack_vertices)
        self.m_scene = scene
        self.m_pRender.set_scene(scene)
        self.resetFrame()

    # sample_example.cpp:103-111 (the image arrives decoded: stbi_loadf has no counterpart here)
    def loadEnvironmentHdr(self, env):
        """SampleExample::loadEnvironmentHdr (sample_example.cpp:102-112): `env` is the path of a Radiance .hdr file (decoded by
        pt_hdr_load, the stbi_loadf of hdr_sampling.cpp:64) or an (h, w, 4) float32 array."""
        env_rgba32f = capi.load_hdr(env) if isinstance(env, (str, bytes, os.PathLike)) else env
        integral, _ = self.m_pRender.set_env(env_rgba32f)
        self.m_rtxState.fireflyClampThreshold = integral * 4.0  # "magic", sample_example.cpp:110
        self.resetFrame()

    def setRenderRegion(self, width, height):
        self.m_size = (int(width), int(height))
        self.m_pRender.create(self.m_size)
        self.resetFrame()

    def _render_size(self):
        """sample_example.cpp:410-413: the size actually rendered (integer division by the de-scaling level while a mouse button is down)"""
        if self.m_descaling:
            return (max(1, self.m_size[0] // self.m_descalingLevel), max(1, self.m_size[1] // self.m_descalingLevel))
        return self.m_size

    # sample_example.cpp:168-178 (the aspect ratio is the render region's, whatever the de-scaling)
    def updateUniformBuffer(self):
        cam = capi.camera_lookat(self.m_scene.camera, self.m_size[0] / self.m_size[1], nb_lights=len(self.m_scene.lights))
        self.m_pRender.set_camera(cam)
        self.m_pRender.set_sunsky(self.m_sunAndSky)

    # sample_example.cpp:183-199: "If the camera matrix has changed, resets the frame otherwise, increments frame."  CameraManip.getMatrix() is
    # the view matrix of (eye, center, up); comparing the three vectors it is computed from is the same predicate.
    def updateFrame(self):
        c = self.m_scene.camera if self.m_scene is not None else None
        m = None if c is None else (tuple(float(x) for x in c.eye), tuple(float(x) for x in c.center), tuple(float(x) for x in c.up))
        f = 0.0 if c is None else float(c.fov)
        if self._refCamMatrix != m or self._refFov != f:
            self.resetFrame()
            self._refCamMatrix, self._refFov = m, f
        if self.m_rtxState.frame < self.m_maxFrames:
            self.m_rtxState.frame += 1

    def resetFrame(self):  # sample_example.cpp:204-207
        self.m_rtxState.frame = -1

    # sample_example.cpp:528-541 / :546-557 -- the de-scaling state machine of the window callbacks
    def onMouseMotion(self, x=0, y=0):
        if self._inputs["lmb"] or self._inputs["rmb"] or self._inputs["mmb"]:
            self.m_descaling = True

    def onMouseButton(self, button, pressed):
        """button: "lmb" | "mmb" | "rmb"; pressed: GLFW_PRESS (True) / GLFW_RELEASE (False)"""
        self._inputs[button] = bool(pressed)
        if not (self._inputs["lmb"] or self._inputs["rmb"] or self._inputs["mmb"]) and not pressed and self.m_descaling:
            self.m_descaling = False
            self.resetFrame()

    # sample_example.cpp:390-429
    def renderScene(self):
        if self.m_rtxState.frame >= self.m_maxFrames:
            return
        size = self._render_size()
        self.m_rtxState.size[0], self.m_rtxState.size[1] = size
        self.m_pRender.setPushContants(self.m_rtxState)
        self.m_pRender.run(None, size, None, None)

    # sample_example.cpp:362-384 -> RenderOutput::run; :378 `zoom = m_descaling ? 1.0f / m_descalingLevel : 1.0f`
    def drawPost(self):
        """The display pass (SampleExample::drawPost, src/sample_example.cpp:396-431).  m_framesInFlight = 0: the RGBA8 image of the frame just
        rendered (the host waits for it).  m_framesInFlight = k > 0: the pass is enqueued and the image of the frame rendered k calls ago is
        returned (None for the first k calls) -- the host never waits for the frame it just issued, like the reference's loop around
        prepareFrame / submitFrame (src/main.cpp:213,261); flushDisplay() returns what is still in flight."""
        size = None
        if self.m_descaling:
            self.m_tonemapper.zoom = 1.0 / self.m_descalingLevel
            size = self.m_size
        else:
            self.m_tonemapper.zoom = 1.0
        if self.m_framesInFlight <= 0:
            return self.m_pRender.tonemap(self.m_tonemapper, display_size=size)
        self.m_pRender.tonemap_begin(self.m_tonemapper, display_size=size)
        if self.m_pRender.tonemap_pending() > min(self.m_framesInFlight, capi.PT_DISPLAY_RING - 1):
            return self.m_pRender.tonemap_end()
        return None

    def flushDisplay(self):
        return [self.m_pRender.tonemap_end() for _ in range(self.m_pRender.tonemap_pending())]

    def render(self, frames):
        """`frames` iterations of the reference's main loop body (src/main.cpp:201-264)."""
        self.updateUniformBuffer()
        for _ in range(frames):
            self.updateFrame()
            self.renderScene()
        self.m_pRender.synchronize()
        return self.m_pRender.read_accum()

    def destroy(self):
        self.m_pRender.destroy()
