"""One Lighting pass worth of inputs (planes, side tables, uniform blocks) and its `sah_lighting_desc` — input plumbing
shared by bench.py, tools/ and tests/.  The same object describes itself over host arrays (numpy) or device arrays (torch)."""
import ctypes as C
import hashlib
import math

import numpy as np

from . import _abi, images, scene, synth


def to_torch(a, device="cuda"):
    import torch
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(device)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).to(device)
    return torch.from_numpy(a).to(device)


def from_torch(t, dtype):
    return t.cpu().numpy().view(dtype)


class LightingInputs:
    def __init__(self, width, height, gbuffer=None, seed=1, sun_mode=_abi.SHADOW_MODE_RT, gi=_abi.GI_NONE, sky=True, flavour="random",
                 flags=_abi.LIGHTING_DEFAULT_FLAGS, shadowmap_res=256, lights=None, cache_debug_mode=0, num_extra_rays=0, synth_device="cpu",
                 shadow="noise"):
        self.width, self.height = width, height
        self.view = scene.SceneView.default(width, height)
        self.sun = scene.DirectionalLight(shadow_mode=sun_mode)
        self.sun_mode = sun_mode
        self.flags = flags
        self.gi_kind = gi
        if gbuffer is None:
            gbuffer = (synth.random_gbuffer(width, height, seed) if flavour == "random"
                       else synth.atrium_gbuffer(width, height, self.view, seed, device=synth_device))
        self.arrays = dict(gbuffer)
        self.arrays["ao"] = synth.ao_plane(width, height, seed + 100)
        self.has_sky = sky
        if sky:
            luts = synth.sky_luts(seed + 200)
            self.arrays["sky_t"] = luts["transmittance"]
            self.arrays["sky_v"] = luts["sky_view"]
        if sun_mode == _abi.SHADOW_MODE_CSM:
            self.sun.update_shadow_cascades(self.view, resolution=shadowmap_res)
            if shadow == "scene" and flavour == "atrium":  # depth of the atrium's own boxes as seen from the sun
                self.arrays["shadowmap"] = synth.atrium_shadowmap(self.sun.constants, shadowmap_res, 4, device=synth_device)
            else:  # D16 noise in [0.3, 0.7]
                self.arrays["shadowmap"] = synth.shadowmap(shadowmap_res, 4, seed + 300)
        if sun_mode == _abi.SHADOW_MODE_RT:
            self.arrays["shadow_mask"] = synth.shadow_mask(width, height, seed + 400)
        self.lpv = None
        if gi == _abi.GI_LPV:
            self.lpv = scene.LpvCascades()
            self.lpv.update_cascade_transforms(self.view, self.sun)
            r, g, b = synth.lpv_volumes(4, seed + 500)
            self.arrays["lpv_r"], self.arrays["lpv_g"], self.arrays["lpv_b"] = r, g, b
        if gi == _abi.GI_CACHE:
            at = synth.probe_atlases(seed + 600)
            self.arrays["probe_irr"], self.arrays["probe_depth"], self.arrays["probe_val"] = at["irradiance"], at["depth"], at["validity"]
        if gi == _abi.GI_RTGI:
            rt = synth.rtgi_planes(width, height, seed + 700)
            self.arrays["ray_buffer"], self.arrays["ray_irr"], self.arrays["noise"] = rt["ray_buffer"], rt["ray_irradiance"], rt["noise"]
        self.cache_debug_mode = cache_debug_mode
        self.num_extra_rays = num_extra_rays
        self.lights = lights  # (N, 8) float32 or None
        if lights is not None:
            self.arrays["lights"] = np.ascontiguousarray(lights, dtype=np.float32)
        self.row_begin = self.row_end = 0

    def bytes_per_pixel(self):
        """Algorithmic plane traffic of one pass: G-buffer 24 B read + lit 8 B written, plus the per-pixel
        input planes the selected sub-passes read (AO 4 — LPV overlay only, shadow mask 4, RTGI ray buffer 8 + irradiance 8)."""
        b = 24 + 8
        if self.gi_kind == _abi.GI_LPV:
            b += 4
        if self.sun_mode == _abi.SHADOW_MODE_RT:
            b += 4
        if self.gi_kind == _abi.GI_RTGI:
            b += 16
        return b

    def describe(self, arrays, lit):
        """Build a LightingDesc over `arrays` (numpy or torch, same keys) writing into `lit`. Returns (desc, keepalive)."""
        keep = []
        gb = images.gbuffer(arrays)
        lit_p = images.plane(lit, _abi.FORMAT_R16G16B16A16_SFLOAT)
        ao_p = images.plane(arrays["ao"], _abi.FORMAT_R32_SFLOAT)
        d = _abi.LightingDesc()
        d.gbuffer = C.pointer(gb)
        d.lit = C.pointer(lit_p)
        d.ao = C.pointer(ao_p)
        d.view = C.pointer(self.view.gpu_data)
        d.sun = C.pointer(self.sun.constants)
        keep += [gb, lit_p, ao_p]
        if "shadowmap" in arrays:
            sm = images.volume(arrays["shadowmap"], _abi.FORMAT_D16_UNORM)
            d.shadowmap = C.pointer(sm)
            keep.append(sm)
        if "shadow_mask" in arrays:
            m = images.plane(arrays["shadow_mask"], _abi.FORMAT_R32_SFLOAT)
            d.shadow_mask = C.pointer(m)
            keep.append(m)
        if self.has_sky:
            sk = _abi.SkyLuts(images.plane(arrays["sky_t"], _abi.FORMAT_R16G16B16A16_SFLOAT),
                              images.plane(arrays["sky_v"], _abi.FORMAT_R16G16B16A16_SFLOAT))
            d.sky = C.pointer(sk)
            keep.append(sk)
        if self.gi_kind != _abi.GI_NONE:
            gi = _abi.GI()
            gi.kind = self.gi_kind
            if self.gi_kind == _abi.GI_LPV:
                gi.lpv_red = images.volume(arrays["lpv_r"], _abi.FORMAT_R16G16B16A16_SFLOAT)
                gi.lpv_green = images.volume(arrays["lpv_g"], _abi.FORMAT_R16G16B16A16_SFLOAT)
                gi.lpv_blue = images.volume(arrays["lpv_b"], _abi.FORMAT_R16G16B16A16_SFLOAT)
                gi.lpv_cascades = C.cast(self.lpv.matrices, C.POINTER(_abi.LpvCascadeMatrices))
                gi.lpv_num_cascades = getattr(self, "lpv_num_cascades", 4)  # (volumes are (32 * cascades) x 32 x 32)
                gi.lpv_exposure = float(np.float32(math.pi) * np.float32(10.0))
                gi.lpv_generation = getattr(self, "lpv_generation", 0)  # 0: the library rebuilds its gather copy of the volumes on every call
            elif self.gi_kind == _abi.GI_CACHE:
                gi.probe_irradiance = images.volume(arrays["probe_irr"], _abi.FORMAT_B10G11R11_UFLOAT_PACK32)
                gi.probe_depth = images.volume(arrays["probe_depth"], _abi.FORMAT_R16G16_SFLOAT)
                gi.probe_validity = images.volume(arrays["probe_val"], _abi.FORMAT_R8_UNORM)
                for c, (cmin, spacing) in enumerate(self.probe_cascades()):
                    gi.probe_cascades[c].probe_spacing = spacing
                    for i in range(3):
                        gi.probe_cascades[c].min[i] = cmin[i]
                gi.probe_size[0], gi.probe_size[1] = 5, 6  # irradiance_cache.cpp:298-299
                gi.cache_debug_mode = self.cache_debug_mode
                gi.probe_generation = getattr(self, "probe_generation", 0)  # 0: the library rebuilds its fp32 gather copy on every call
            elif self.gi_kind == _abi.GI_RTGI:
                gi.ray_buffer = images.plane(arrays["ray_buffer"], _abi.FORMAT_R16G16B16A16_SFLOAT)
                gi.ray_irradiance = images.plane(arrays["ray_irr"], _abi.FORMAT_R16G16B16A16_SFLOAT)
                gi.noise = images.plane(arrays["noise"], _abi.FORMAT_R8G8B8A8_UNORM)
                gi.num_extra_rays = self.num_extra_rays
                gi.extra_ray_radius = 16.0
            d.gi = C.pointer(gi)
            keep.append(gi)
        if self.lights is not None:
            la = arrays["lights"]
            ptr = la.ctypes.data if isinstance(la, np.ndarray) else la.data_ptr()
            ll = _abi.LightList(ptr, self.lights.shape[0])
            d.lights = C.pointer(ll)
            keep.append(ll)
        d.flags = self.flags
        d.row_begin, d.row_end = self.row_begin, self.row_end
        keep.append(arrays)
        return d, keep

    def probe_cascades(self):
        """Stand-in placement of the four irradiance-cache cascades: centred on the camera, spacing 0.5 m doubling per cascade.
        Returns [(min xyz, spacing)] as Python floats (the ABI struct rounds them to fp32)."""
        pos = self.view.position
        out = []
        for c in range(4):
            spacing = 0.5 * (2.0 ** c)
            ext = (32 * spacing, 8 * spacing, 32 * spacing)
            out.append(([float(pos[i]) - ext[i] / 2.0 + 0.013 * (c + 1) for i in range(3)], spacing))
        return out

    def inputs_sha256(self):
        m = hashlib.sha256()
        for k in sorted(self.arrays):
            m.update(k.encode())
            m.update(np.ascontiguousarray(self.arrays[k]).tobytes())
        return m.hexdigest()

    def device_arrays(self, device="cuda"):
        return {k: to_torch(v, device) for k, v in self.arrays.items()}

    def run_hip(self, ctx, dev=None):
        import torch
        dev = dev or self.device_arrays()
        lit = torch.zeros((self.height, self.width, 4), dtype=torch.int16, device="cuda")
        d, keep = self.describe(dev, lit)
        ctx.lighting(d)
        torch.cuda.synchronize()
        return from_torch(lit, np.uint16)


def rasterised_frame(ctx, geometry, view_data, gbuffer, motion_vectors=None, stats_ptr=None, vrsaa=None, fused_motion=False, sun_shafts=None,
                     translucent=None):
    """The rasterised part of a frame: sah_gbuffer_render into `gbuffer` (dict of device arrays: color, normals, data, emission, depth)
    and — only when a `motion_vectors` target (H, W, 2) int16 device array is given — sah_motion_vectors_render against the depth the
    G-buffer pass has just written, as the reference runs its motion-vectors phase after its depth pass (scene_renderer.cpp:308-316).
    Without the target the frame is what it always was.  `fused_motion` (off by default) with a target: the two passes as the one call
    sah_gbuffer_motion_render, which gives the same bytes with one rasteriser set-up (include/sah_gbuffer_motion.h).

    `vrsaa` (off by default): a dict with "rates" [(x, y), ...] and "texel_size" (x, y), and optionally the device arrays "contrast"
    (H, W, 2) int16 — the LAST frame's contrast image — and "shading_rate_image" (uint8, the extent of
    scene.shading_rate_image_extent); missing arrays are created, zeroed.  In the reference's order (scene_renderer.cpp:357-361, 476-481):
    the shading-rate image is made from the previous contrast image before the G-buffer pass, and this frame's contrast is measured into the
    same array at the end, from the G-buffer's colour and depth.  Returns (contrast, shading_rate_image) then, None otherwise.

    `sun_shafts` (off by default): a dict with "pass" (a SunShafts), "sun" (the sah_sun_light_constants) and "shadowmap" (the cascades' device
    array, or None), and optionally "lit", the (H, W, 4) int16 image Lighting made of an earlier G-buffer of this extent.  The volumetric sun
    light is marched against the depth the G-buffer pass has just written — its place between Lighting and the anti-aliasing — and the
    plane it returns is stored under "out".  Without "lit" the pass must carry SUN_SHAFTS_TERM_ONLY: "out" is then the term (S, T) for the
    caller to apply once Lighting has run.

    `translucent` (off by default): a dict with "pass" (a Translucency), "geometry" (the sah_scene_geometry of the translucent primitives,
    back to front) and "lighting" (a callable taking the G-buffer dict this function has just filled and returning the frame's
    sah_lighting_desc — or (desc, keepalive) — over it, its `lit` plane being the image to end up in).  `geometry`, the positional argument,
    is then the scene WITHOUT its type-2 primitives (mesh.split_translucent): the G-buffer and motion-vectors passes see the opaque half
    only, as sah_rt_build must.  After the raster passes the frame's Lighting pass runs — sah_lighting with that descriptor — and the
    translucent primitives are blended into its `lit` (include/sah_translucent.h), before the sun shafts."""
    sri = contrast = None
    if vrsaa is not None:
        import torch
        h, w = gbuffer["depth"].shape[0], gbuffer["depth"].shape[1]
        sw, sh = scene.shading_rate_image_extent((w, h), vrsaa["texel_size"])
        contrast = vrsaa.get("contrast")
        if contrast is None:
            contrast = torch.zeros((h, w, 2), dtype=torch.int16, device=gbuffer["depth"].device)
        sri = vrsaa.get("shading_rate_image")
        if sri is None:
            sri = torch.zeros((sh, sw), dtype=torch.uint8, device=gbuffer["depth"].device)
        contrast_p = images.plane(contrast, _abi.FORMAT_R16G16_SFLOAT)
        ctx.vrsaa_shading_rate_image(contrast_p, images.plane(sri, _abi.FORMAT_R8_UINT), scene.shading_rate_params((w, h), (sw, sh), vrsaa["rates"]))
    if fused_motion and motion_vectors is not None:
        ctx.gbuffer_motion_render(geometry, view_data, images.gbuffer(gbuffer), images.plane(motion_vectors, _abi.FORMAT_R16G16_SFLOAT), stats_ptr)
    else:
        ctx.gbuffer_render(geometry, view_data, images.gbuffer(gbuffer), stats_ptr)
    if motion_vectors is not None and not fused_motion:
        ctx.motion_vectors_render(geometry, view_data, images.plane(gbuffer["depth"], _abi.FORMAT_D32_SFLOAT),
                                  images.plane(motion_vectors, _abi.FORMAT_R16G16_SFLOAT))
    if translucent is not None:
        made = translucent["lighting"](gbuffer)
        desc, translucent["keep"] = made if isinstance(made, tuple) else (made, None)
        ctx.lighting(desc)
        translucent["pass"](desc, translucent["geometry"])
    if sun_shafts is not None:
        sun_shafts["out"] = sun_shafts["pass"](view_data, sun_shafts["sun"], sun_shafts.get("shadowmap"), gbuffer["depth"], sun_shafts.get("lit"))
    if vrsaa is not None:
        ctx.vrsaa_measure_aliasing(images.plane(gbuffer["color"], _abi.FORMAT_R8G8B8A8_SRGB), images.plane(gbuffer["depth"], _abi.FORMAT_D32_SFLOAT), contrast_p)
        return contrast, sri
    return None


class TemporalResolver:
    """Temporal anti-aliasing over successive frames (include/sah_taa.h): owns the two ping-pong targets — this frame's output is the next
    frame's history — and the previous frame's jitter.  The first frame, and the first after reset() (a camera cut), passes
    SAH_TAA_HISTORY_INVALID: the output is then the lit frame."""

    def __init__(self, ctx, width, height, blend=0.1, hdr_weights=True, device="cuda"):
        import torch
        self.ctx, self.width, self.height, self.blend, self.hdr_weights = ctx, width, height, blend, hdr_weights
        self.targets = [torch.zeros((height, width, 4), dtype=torch.int16, device=device) for _ in range(2)]
        self.current = 0  # index of the target the last resolve() wrote
        self.previous_jitter = (0.0, 0.0)
        self.history_valid = False

    def reset(self):
        self.history_valid = False

    def resolve(self, lit, depth, motion_vectors, jitter, rows=(0, 0)):
        """lit (H, W, 4) int16, depth (H, W) float32, motion_vectors (H, W, 2) int16 device arrays, `jitter` the (x, y) this frame was rendered
        with.  Returns the resolved frame: one of the two targets, valid until the call after the next."""
        params = _abi.TaaParams()
        params.blend = self.blend
        params.jitter[:] = [float(jitter[0]), float(jitter[1])]
        params.previous_jitter[:] = self.previous_jitter if self.history_valid else params.jitter[:]
        params.flags = (_abi.TAA_HDR_WEIGHTS if self.hdr_weights else 0) | (0 if self.history_valid else _abi.TAA_HISTORY_INVALID)
        history, out = self.targets[self.current], self.targets[1 - self.current]
        self.ctx.taa_resolve(images.plane(lit, _abi.FORMAT_R16G16B16A16_SFLOAT), images.plane(depth, _abi.FORMAT_D32_SFLOAT),
                             images.plane(motion_vectors, _abi.FORMAT_R16G16_SFLOAT),
                             images.plane(history, _abi.FORMAT_R16G16B16A16_SFLOAT) if self.history_valid else None,
                             images.plane(out, _abi.FORMAT_R16G16B16A16_SFLOAT), params, rows)
        self.current = 1 - self.current
        self.previous_jitter = (params.jitter[0], params.jitter[1])
        self.history_valid = True
        return out


class TemporalUpscaler:
    """Temporal upscaling over successive frames (include/sah_taa_upscale.h): the frame is rendered, jittered, at `render` and resolved to
    `output`.  Owns the two ping-pong targets of the output extent and the previous frame's jitter, like TemporalResolver.  The first frame,
    and the first after reset() (a camera cut), passes SAH_TAA_HISTORY_INVALID: the output is then the bilinear upsample of the lit frame."""

    def __init__(self, ctx, render, output, blend=0.1, min_confidence=0.05, hdr_weights=True, device="cuda"):
        import torch
        self.ctx, self.render, self.output = ctx, tuple(render), tuple(output)
        self.blend, self.min_confidence, self.hdr_weights = blend, min_confidence, hdr_weights
        self.targets = [torch.zeros((self.output[1], self.output[0], 4), dtype=torch.int16, device=device) for _ in range(2)]
        self.current = 0  # index of the target the last resolve() wrote
        self.previous_jitter = (0.0, 0.0)
        self.history_valid = False

    def reset(self):
        self.history_valid = False

    def resolve(self, lit, depth, motion_vectors, jitter, rows=(0, 0)):
        """lit (h, w, 4) int16, depth (h, w) float32, motion_vectors (h, w, 2) int16 device arrays of the render extent, `jitter` the (x, y)
        in render pixels this frame was rendered with.  Returns the resolved (H, W, 4) frame: one of the two targets, valid until the call
        after the next."""
        params = _abi.TaaUpscaleParams()
        params.blend, params.min_confidence = self.blend, self.min_confidence
        params.jitter[:] = [float(jitter[0]), float(jitter[1])]
        params.previous_jitter[:] = self.previous_jitter if self.history_valid else params.jitter[:]
        params.flags = (_abi.TAA_HDR_WEIGHTS if self.hdr_weights else 0) | (0 if self.history_valid else _abi.TAA_HISTORY_INVALID)
        history, out = self.targets[self.current], self.targets[1 - self.current]
        self.ctx.taa_upscale(images.plane(lit, _abi.FORMAT_R16G16B16A16_SFLOAT), images.plane(depth, _abi.FORMAT_D32_SFLOAT),
                             images.plane(motion_vectors, _abi.FORMAT_R16G16_SFLOAT),
                             images.plane(history, _abi.FORMAT_R16G16B16A16_SFLOAT) if self.history_valid else None,
                             images.plane(out, _abi.FORMAT_R16G16B16A16_SFLOAT), params, rows)
        self.current = 1 - self.current
        self.previous_jitter = (params.jitter[0], params.jitter[1])
        self.history_valid = True
        return out


class ScreenSpaceAO:
    """Screen-space ambient occlusion (include/sah_ssao.h) for frames of one extent: owns the AO plane sah_lighting reads and the scratch plane
    of the raw, unblurred result, which the library does not allocate.  `settings` are fields of _abi.SsaoParams; the defaults are the
    reference's CACAO settings."""

    def __init__(self, ctx, width, height, device="cuda", **settings):
        import torch
        self.ctx, self.width, self.height = ctx, width, height
        self.params = _abi.SsaoParams.default(**settings)
        self.ao = torch.ones((height, width), dtype=torch.float32, device=device)
        self.scratch = torch.ones((height, width), dtype=torch.float32, device=device)

    def generate(self, view_data, depth, normals, rows=(0, 0)):
        """depth (H, W) float32 and normals (H, W, 4) int16 device arrays (the G-buffer's), view_data the frame's _abi.ViewData.  Returns the
        AO plane, (H, W) float32: the same array every call."""
        scratch = images.plane(self.scratch, _abi.FORMAT_R32_SFLOAT) if self.params.blur_passes else None
        self.ctx.ssao(view_data, images.plane(depth, _abi.FORMAT_D32_SFLOAT), images.plane(normals, _abi.FORMAT_R16G16B16A16_SFLOAT), scratch,
                      images.plane(self.ao, _abi.FORMAT_R32_SFLOAT), self.params, rows)
        return self.ao


def adaptation_from(dt, speed):
    """The `adaptation` weight of a frame that took `dt` seconds at `speed` per second: 1 - exp(-dt * speed), clamped into (0, 1]."""
    a = 1.0 - math.exp(-float(dt) * float(speed))
    return min(max(a, float(np.finfo(np.float32).tiny)), 1.0)


class AutoExposure:
    """Histogram auto-exposure (include/sah_exposure.h) over successive frames: owns the histogram's work buffer, the two ping-ponged states
    and the exposed plane, which is re-created (and the history dropped) when a scene of another extent arrives.  The first frame, and the first after reset() (a cut), is metered and then exposed by its own
    exposure (sah_exposure_meter with SAH_EXPOSURE_HISTORY_INVALID, then sah_exposure_apply); later frames take the fused call and are
    exposed by what the frame before metered.  `settings` are fields of _abi.ExposureParams; set `params.adaptation` per frame from
    adaptation_from(dt, speed)."""

    def __init__(self, ctx, width, height, device="cuda", **settings):
        import torch
        self.ctx, self.width, self.height = ctx, width, height
        self.params = _abi.ExposureParams.default(**settings)
        self.work = torch.zeros(260, dtype=torch.int32, device=device)  # SAH_EXPOSURE_WORK_BYTES
        self.states = [torch.zeros(4, dtype=torch.float32, device=device) for _ in range(2)]
        self.exposed = torch.zeros((height, width, 4), dtype=torch.int16, device=device)
        self.current = 0  # index of the state the last expose() wrote
        self.history_valid = False

    def reset(self):
        self.history_valid = False

    def state(self):
        """the state the last expose() wrote, as an _abi.ExposureState (synchronises)"""
        return _abi.ExposureState.from_buffer_copy(self.states[self.current].cpu().numpy().tobytes())

    def histogram(self):
        """the last frame's 256-bin histogram (synchronises)"""
        return self.work[:256].cpu().numpy().view(np.uint32)

    def expose(self, scene):
        """scene (H, W, 4) int16 device array.  Returns the exposed plane, (H, W, 4) int16: the same array every call."""
        p = self.params
        if tuple(scene.shape[:2]) != (self.height, self.width):  # another extent: a new exposed plane, and no history
            import torch
            self.height, self.width = int(scene.shape[0]), int(scene.shape[1])
            self.exposed = torch.zeros((self.height, self.width, 4), dtype=torch.int16, device=self.exposed.device)
            self.history_valid = False
        scene_p, out_p = images.plane(scene, _abi.FORMAT_R16G16B16A16_SFLOAT), images.plane(self.exposed, _abi.FORMAT_R16G16B16A16_SFLOAT)
        old, new = self.current, 1 - self.current
        if self.history_valid:
            p.flags &= ~_abi.EXPOSURE_HISTORY_INVALID
            self.ctx.exposure_meter(scene_p, self.states[old].data_ptr(), self.states[new].data_ptr(), self.work.data_ptr(), out_p, p)
        else:
            p.flags |= _abi.EXPOSURE_HISTORY_INVALID
            self.ctx.exposure_meter(scene_p, None, self.states[new].data_ptr(), self.work.data_ptr(), None, p)
            self.ctx.exposure_apply(scene_p, self.states[new].data_ptr(), out_p)
        self.current = new
        self.history_valid = True
        return self.exposed


class Sharpener:
    """Contrast-adaptive sharpening (include/sah_sharpen.h) behind the upscale: owns the sharpened plane, which is re-created when a scene of
    another extent arrives.  `settings` are fields of _abi.SharpenParams."""

    def __init__(self, ctx, width, height, device="cuda", **settings):
        import torch
        self.ctx, self.width, self.height = ctx, width, height
        self.params = _abi.SharpenParams.default(**settings)
        self.sharpened = torch.zeros((height, width, 4), dtype=torch.int16, device=device)

    def sharpen(self, scene, exposure_state=None, rows=(0, 0)):
        """scene (H, W, 4) int16 device array; exposure_state the data_ptr() of a 16-byte exposure state (AutoExposure's), or None.  Returns
        the sharpened plane, (H, W, 4) int16: the same array every call while the extent stays."""
        if tuple(scene.shape[:2]) != (self.height, self.width):
            import torch
            self.height, self.width = int(scene.shape[0]), int(scene.shape[1])
            self.sharpened = torch.zeros((self.height, self.width, 4), dtype=torch.int16, device=self.sharpened.device)
        self.ctx.sharpen(images.plane(scene, _abi.FORMAT_R16G16B16A16_SFLOAT), exposure_state, images.plane(self.sharpened, _abi.FORMAT_R16G16B16A16_SFLOAT),
                         self.params, rows)
        return self.sharpened


class ScreenSpaceReflections:
    """Screen-space reflections (include/sah_ssr.h) between Lighting and the anti-aliasing: owns the plane with the reflections added and the
    scratch plane of one float per 8 x 8 block (reserved by the header, not touched yet), both re-created when a frame of another extent arrives.  `settings` are fields of _abi.SsrParams.  Off
    by default: nothing creates one but the caller that wants reflections."""

    def __init__(self, ctx, width, height, device="cuda", **settings):
        self.ctx, self.device = ctx, device
        self.params = _abi.SsrParams.default(**settings)
        self._allocate(width, height)

    def _allocate(self, width, height):
        import torch
        self.width, self.height = width, height
        self.out = torch.zeros((height, width, 4), dtype=torch.int16, device=self.device)
        self.scratch = torch.zeros(((height + 7) // 8, (width + 7) // 8), dtype=torch.float32, device=self.device)

    def __call__(self, view_data, gbuffer, lit, source=None, rows=(0, 0)):
        """gbuffer a dict of device arrays with "color", "normals", "data" and "depth" (the G-buffer's); lit (H, W, 4) int16, the image the
        reflections are added to; source the image they are taken from — lit itself unless given (last frame's output, say: not this
        object's `out`, which the call writes).  Returns the plane with the reflections added, (H, W, 4) int16: the same array every call
        while the extent stays."""
        if tuple(lit.shape[:2]) != (self.height, self.width):
            self._allocate(int(lit.shape[1]), int(lit.shape[0]))
        rgba16 = _abi.FORMAT_R16G16B16A16_SFLOAT
        lit_p = images.plane(lit, rgba16)
        self.ctx.ssr(view_data, images.plane(gbuffer["color"], _abi.FORMAT_R8G8B8A8_SRGB), images.plane(gbuffer["normals"], rgba16),
                     images.plane(gbuffer["data"], _abi.FORMAT_R8G8B8A8_UNORM), images.plane(gbuffer["depth"], _abi.FORMAT_D32_SFLOAT),
                     lit_p if source is None else images.plane(source, rgba16), lit_p, images.plane(self.scratch, _abi.FORMAT_R32_SFLOAT),
                     images.plane(self.out, rgba16), self.params, rows)
        return self.out


class MotionBlur:
    """Camera motion blur (include/sah_motion_blur.h) behind the anti-aliasing and the sharpening and ahead of the exposure: owns the blurred
    plane and the scratch plane of one vector per 16 x 16 tile of the render raster, both re-created when a frame of other extents arrives.
    `settings` are fields of _abi.MotionBlurParams (the jitters are taken per frame).  Tracks the previous frame's jitter like
    TemporalResolver; the first frame, and the first after reset() (a camera cut), takes the previous jitter to be this frame's.  Off by
    default: nothing creates one but the caller that wants the blur."""

    def __init__(self, ctx, width, height, render_width=None, render_height=None, device="cuda", **settings):
        self.ctx, self.device = ctx, device
        self.params = _abi.MotionBlurParams.default(**settings)
        self.reset()
        self._allocate(width, height, width if render_width is None else render_width, height if render_height is None else render_height)

    def _allocate(self, width, height, render_width, render_height):
        import torch
        self.width, self.height, self.render_width, self.render_height = width, height, render_width, render_height
        self.out = torch.zeros((height, width, 4), dtype=torch.int16, device=self.device)
        self.tiles = torch.zeros(((render_height + 15) // 16, (render_width + 15) // 16, 2), dtype=torch.int16, device=self.device)

    def reset(self):
        self.history_valid = False
        self.previous_jitter = (0.0, 0.0)

    def __call__(self, scene, depth, motion_vectors, jitter=(0.0, 0.0), z_near=None, rows=(0, 0)):
        """scene (H, W, 4) int16 of the output extent; depth (h, w) float32 and motion_vectors (h, w, 2) int16 of the render extent, device
        arrays; `jitter` the (x, y) this frame was rendered with, z_near the view's (the parameters' unless given).  Returns the blurred
        plane, (H, W, 4) int16: the same array every call while the extents stay."""
        extents = (int(scene.shape[1]), int(scene.shape[0]), int(depth.shape[1]), int(depth.shape[0]))
        if extents != (self.width, self.height, self.render_width, self.render_height):
            self._allocate(*extents)
        p = self.params
        if z_near is not None:
            p.z_near = float(z_near)
        p.jitter[:] = [float(jitter[0]), float(jitter[1])]
        p.previous_jitter[:] = self.previous_jitter if self.history_valid else p.jitter[:]
        rgba16, rg16 = _abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_R16G16_SFLOAT
        self.ctx.motion_blur(images.plane(scene, rgba16), images.plane(depth, _abi.FORMAT_D32_SFLOAT), images.plane(motion_vectors, rg16),
                             images.plane(self.tiles, rg16), images.plane(self.out, rgba16), p, rows)
        self.previous_jitter = (p.jitter[0], p.jitter[1])
        self.history_valid = True
        return self.out


class SunShafts:
    """Volumetric sun light (include/sah_sun_shafts.h) between Lighting and the anti-aliasing: owns the plane with the shafts added and the
    march plane, both re-created when a frame of another extent arrives or params.downscale was changed, and forms step_transmittance = exp(-extinction * step_length) —
    the library itself never evaluates an exponential.  `settings` are fields of _abi.SunShaftsParams; unless given, the albedo is
    Lighting's exposure constant (a white medium in lit's units).  Under SUN_SHAFTS_DITHER the dither offset steps by one every call, so
    that a temporal resolve behind the pass averages the sixteen offsets.  Off by default: nothing creates one but the caller that wants
    the shafts."""

    def __init__(self, ctx, width, height, extinction=0.04, device="cuda", **settings):
        self.ctx, self.device = ctx, device
        settings.setdefault("albedo", (_abi.LIGHTING_EXPOSURE,) * 3)
        given = "step_transmittance" in settings
        self.params = _abi.SunShaftsParams.default(**settings)
        self.extinction = None if given else extinction
        if not given:
            self.set_extinction(extinction)
        self.calls = 0
        self._allocate(width, height)

    def set_extinction(self, extinction):
        """extinction coefficient of the medium per view-space unit, >= 0"""
        self.extinction = float(extinction)
        self.params.step_transmittance = math.exp(-self.extinction * self.params.step_length)

    def _allocate(self, width, height):
        import torch
        s = self.downscale = int(self.params.downscale)
        self.width, self.height = width, height
        self.out = torch.zeros((height, width, 4), dtype=torch.int16, device=self.device)
        self.march = torch.zeros(((height + s - 1) // s, (width + s - 1) // s, 4), dtype=torch.int16, device=self.device)

    def __call__(self, view_data, sun, shadowmap, depth, lit=None, rows=(0, 0)):
        """depth (h, w) float32 and lit (h, w, 4) int16 (None under SUN_SHAFTS_TERM_ONLY) device arrays; shadowmap the cascades as a
        (layers, H, W) device array, int16 for D16_UNORM or float32 for D32_SFLOAT, or None (every sample lit).  Returns the plane with the
        shafts added, (h, w, 4) int16: the same array every call while the extent stays."""
        import torch
        p = self.params
        if (int(depth.shape[1]), int(depth.shape[0]), int(p.downscale)) != (self.width, self.height, self.downscale):  # (params may be changed between calls)
            self._allocate(int(depth.shape[1]), int(depth.shape[0]))
        p.dither_offset = self.calls & 15 if p.flags & _abi.SUN_SHAFTS_DITHER else p.dither_offset
        self.calls += 1
        rgba16 = _abi.FORMAT_R16G16B16A16_SFLOAT
        volume = None
        if shadowmap is not None:
            volume = images.volume(shadowmap, _abi.FORMAT_D32_SFLOAT if shadowmap.dtype == torch.float32 else _abi.FORMAT_D16_UNORM)
        self.ctx.sun_shafts(view_data, sun, volume, images.plane(depth, _abi.FORMAT_D32_SFLOAT), None if lit is None else images.plane(lit, rgba16),
                            images.plane(self.march, rgba16), images.plane(self.out, rgba16), p, rows)
        return self.out


class Translucency:
    """Alpha-blended geometry over the lit scene (include/sah_translucent.h), after Lighting (and after the screen-space reflections, where
    they write into lit's place) and before the sun shafts and the anti-aliasing.  Owns the statistics words of the last call.  Calling it
    blends the primitives of type PRIMITIVE_TYPE_TRANSLUCENT of `geometry` — the translucent half of mesh.split_translucent, ordered by
    mesh.sort_back_to_front — into the `lit` plane of `lighting_desc`, the frame's own _abi.LightingDesc, each fragment lit by that
    descriptor.  Off by default: nothing creates one but the caller that wants translucent geometry drawn."""

    def __init__(self, ctx, device="cuda"):
        import torch
        self.ctx = ctx
        self.stats = torch.zeros(_abi.RASTER_STATS_WORDS, dtype=torch.int32, device=device)

    def __call__(self, lighting_desc, geometry, rows=None):
        """rows: (begin, end) to blend a band of the frame only (None: the descriptor's own range)"""
        if rows is not None:
            saved = lighting_desc.row_begin, lighting_desc.row_end
            lighting_desc.row_begin, lighting_desc.row_end = rows
        try:
            self.ctx.translucent_render(lighting_desc, geometry, self.stats.data_ptr())
        finally:
            if rows is not None:
                lighting_desc.row_begin, lighting_desc.row_end = saved

    def deepest_pixel(self):
        """the most fragments the last call blended at one pixel (a read-back: synchronises)"""
        return int(self.stats[7].item())


class VrsaaFrame:
    """The lighting half of the reference's own anti-aliasing mode (AntiAliasingType::VRSAA) for an output of width x height
    (include/sah_vrs.h): Lighting at 2W x 2H at the rate the shading-rate image of rasterised_frame(vrsaa=...) asks for, then the resolve to
    W x H.  Owns the two planes.  Off by default: nothing creates one but the caller that selects the mode."""

    def __init__(self, ctx, width, height, texel_size, depth_tolerance=0.01, device="cuda"):
        import torch
        self.ctx, self.width, self.height = ctx, width, height
        self.texel_size, self.depth_tolerance = tuple(texel_size), depth_tolerance
        self.lit = torch.zeros((2 * height, 2 * width, 4), dtype=torch.int16, device=device)
        self.antialiased = torch.zeros((height, width, 4), dtype=torch.int16, device=device)

    def render(self, inputs, arrays, shading_rate_image):
        """inputs: the LightingInputs of the 2W x 2H frame; arrays: its device arrays (inputs.device_arrays(), or the G-buffer the rasteriser
        has just written with the side planes); shading_rate_image: the uint8 device array rasterised_frame(vrsaa=...) returns.  Returns
        antialiased, (H, W, 4) int16: the same array every call."""
        if (inputs.width, inputs.height) != (2 * self.width, 2 * self.height):
            raise ValueError(f"the frame is {inputs.width} x {inputs.height}, not twice {self.width} x {self.height}")
        desc, keep = inputs.describe(arrays, self.lit)
        self.ctx.lighting_vrs(desc, images.plane(shading_rate_image, _abi.FORMAT_R8_UINT), self.texel_size, self.depth_tolerance)
        self.ctx.vrsaa_resolve(images.plane(self.lit, _abi.FORMAT_R16G16B16A16_SFLOAT), images.plane(self.antialiased, _abi.FORMAT_R16G16B16A16_SFLOAT))
        return self.antialiased


class RayTracedDenoiser:
    """The temporal and edge-aware filter for a one-channel ray-traced plane (include/sah_rt_denoise.h) over successive frames of one
    extent: owns the two ping-ponged accumulation / sample-count pairs — this frame's accum_out and length_out are the next frame's history
    — the kept copy of the last frame's depth, and the `denoised` plane sah_lighting reads; tracks the previous jitter and whether there
    is a history, like TemporalResolver.  The first frame, and the first after reset() (a camera cut), passes
    SAH_RT_DENOISE_HISTORY_INVALID.  `settings` are fields of _abi.RtDenoiseParams.  One instance per plane (AO, the sun's mask).  The
    depth is kept with a device copy on torch's current stream, which must be the context's."""

    def __init__(self, ctx, width, height, device="cuda", **settings):
        import torch
        self.ctx, self.width, self.height = ctx, width, height
        self.params = _abi.RtDenoiseParams.default(**settings)
        self.accum = [torch.zeros((height, width), dtype=torch.float32, device=device) for _ in range(2)]
        self.length = [torch.zeros((height, (width + 1) // 2 * 2), dtype=torch.float16, device=device) for _ in range(2)]  # pitch: a multiple of 4
        self.previous_depth = torch.zeros((height, width), dtype=torch.float32, device=device)
        self.denoised = torch.ones((height, width), dtype=torch.float32, device=device)
        self.current = 0  # index of the pair the last denoise() wrote
        self.previous_jitter = (0.0, 0.0)
        self.history_valid = False

    def reset(self):
        self.history_valid = False

    def _length_plane(self, t):
        return _abi.Plane(t.data_ptr(), self.width, self.height, t.shape[1] * 2, _abi.FORMAT_R16_SFLOAT)

    def denoise(self, view_data, noisy, depth, normals, motion_vectors, jitter):
        """noisy and depth (H, W) float32, normals (H, W, 4) int16, motion_vectors (H, W, 2) int16 device arrays of this frame, view_data its
        _abi.ViewData, `jitter` the (x, y) it was rendered with.  Returns the denoised plane, (H, W) float32: the same array every call."""
        p = self.params
        p.jitter[:] = [float(jitter[0]), float(jitter[1])]
        p.previous_jitter[:] = self.previous_jitter if self.history_valid else p.jitter[:]
        p.flags = 0 if self.history_valid else _abi.RT_DENOISE_HISTORY_INVALID
        old, new = self.current, 1 - self.current
        R32F, D32 = _abi.FORMAT_R32_SFLOAT, _abi.FORMAT_D32_SFLOAT
        previous = dict(previous_depth=images.plane(self.previous_depth, D32), history=images.plane(self.accum[old], R32F),
                        history_length=self._length_plane(self.length[old])) if self.history_valid else {}
        desc = _abi.RtDenoiseDesc.of(noisy=images.plane(noisy, R32F), depth=images.plane(depth, D32),
                                     normals=images.plane(normals, _abi.FORMAT_R16G16B16A16_SFLOAT),
                                     motion_vectors=images.plane(motion_vectors, _abi.FORMAT_R16G16_SFLOAT),
                                     accum_out=images.plane(self.accum[new], R32F), length_out=self._length_plane(self.length[new]),
                                     denoised=images.plane(self.denoised, R32F), **previous)
        self.ctx.rt_denoise(view_data, desc, p)
        self.previous_depth.copy_(depth)
        self.current = new
        self.previous_jitter = (p.jitter[0], p.jitter[1])
        self.history_valid = True
        return self.denoised


class RtgiDenoiser:
    """The temporal accumulation and variance-guided filter for the RTGI ray planes (include/sah_rtgi_denoise.h) over successive frames of
    one extent: owns the two ping-ponged accumulation / moments pairs — this frame's accum_out and moments_out are the next frame's history
    — the kept copy of the last frame's depth, and the two denoised planes sah_lighting reads as gi.ray_buffer and gi.ray_irradiance; tracks
    the previous jitter and whether there is a history, like RayTracedDenoiser.  The first frame, and the first after reset() (a camera cut),
    passes SAH_RTGI_DENOISE_HISTORY_INVALID.  `settings` are fields of _abi.RtgiDenoiseParams.  The depth is kept with a device copy on
    torch's current stream, which must be the context's."""

    def __init__(self, ctx, width, height, device="cuda", **settings):
        import torch
        self.ctx, self.width, self.height = ctx, width, height
        self.params = _abi.RtgiDenoiseParams.default(**settings)
        self.accum = [torch.zeros((height, width, 4), dtype=torch.float32, device=device) for _ in range(2)]
        self.moments = [torch.zeros((height, width, 2), dtype=torch.float32, device=device) for _ in range(2)]
        self.previous_depth = torch.zeros((height, width), dtype=torch.float32, device=device)
        self.denoised_ray_buffer = torch.zeros((height, width, 4), dtype=torch.int16, device=device)
        self.denoised_irradiance = torch.zeros((height, width, 4), dtype=torch.int16, device=device)
        self.current = 0  # index of the pair the last denoise() wrote
        self.previous_jitter = (0.0, 0.0)
        self.history_valid = False

    def reset(self):
        self.history_valid = False

    def denoise(self, view_data, ray_buffer, ray_irradiance, depth, normals, motion_vectors, jitter):
        """ray_buffer, ray_irradiance and normals (H, W, 4) int16, depth (H, W) float32, motion_vectors (H, W, 2) int16 device arrays of this
        frame, view_data its _abi.ViewData, `jitter` the (x, y) it was rendered with.  Returns (denoised_ray_buffer, denoised_irradiance),
        (H, W, 4) int16: the same arrays every call."""
        p = self.params
        p.jitter[:] = [float(jitter[0]), float(jitter[1])]
        p.previous_jitter[:] = self.previous_jitter if self.history_valid else p.jitter[:]
        p.flags = 0 if self.history_valid else _abi.RTGI_DENOISE_HISTORY_INVALID
        old, new = self.current, 1 - self.current
        RGBA16F, RGBA32F, RG32F, D32 = _abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_R32G32B32A32_SFLOAT, _abi.FORMAT_R32G32_SFLOAT, _abi.FORMAT_D32_SFLOAT
        previous = dict(previous_depth=images.plane(self.previous_depth, D32), history=images.plane(self.accum[old], RGBA32F),
                        history_moments=images.plane(self.moments[old], RG32F)) if self.history_valid else {}
        desc = _abi.RtgiDenoiseDesc.of(ray_buffer=images.plane(ray_buffer, RGBA16F), ray_irradiance=images.plane(ray_irradiance, RGBA16F),
                                       depth=images.plane(depth, D32), normals=images.plane(normals, RGBA16F),
                                       motion_vectors=images.plane(motion_vectors, _abi.FORMAT_R16G16_SFLOAT),
                                       accum_out=images.plane(self.accum[new], RGBA32F), moments_out=images.plane(self.moments[new], RG32F),
                                       denoised_ray_buffer=images.plane(self.denoised_ray_buffer, RGBA16F),
                                       denoised_irradiance=images.plane(self.denoised_irradiance, RGBA16F), **previous)
        self.ctx.rtgi_denoise(view_data, desc, p)
        self.previous_depth.copy_(depth)
        self.current = new
        self.previous_jitter = (p.jitter[0], p.jitter[1])
        self.history_valid = True
        return self.denoised_ray_buffer, self.denoised_irradiance
