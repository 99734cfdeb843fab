"""Python API of the renderer: ``Scene``, ``Camera``, ``float3`` — the reference's public surface
(/root/reference/render.py:31-257, __init__.py:1) on top of libzdr_hip.so.

    scene = Scene([(obj_path, transform_or_None, emission), ...], integrator="path")
    scene.camera = Camera(fov=..., origin=float3(...), target=float3(...), up=float3(...))
    image = scene.render(material, res=(W, H), spp=256, seed=0)      # (H, W, 4) float32, differentiable
    image.sum().backward()                                            # material.grad: (Ht, Wt, 4)

    scene.material_slots = [0, 1, None]                               # one material per model (None: light or blocker)
    image = scene.render([floor, box], res=(W, H), spp=256)           # floor.grad and box.grad after backward()

    scene.add_envmap(sky)                                             # the map and its importance-sampling tables
    env = torch.tensor(sky, device="cuda", requires_grad=True)        # (H, 2H, 3|4) or (H, H, 3|4)
    image = scene.render(material, res=(W, H), spp=256, envmap=env)   # env.grad after backward(); tables stay fixed
    scene.update_envmap_sampling(None, on_device=True)                # tables rebuilt from the current map, on the GPU and in place

    f = scene.render_aovs(material, res=(W, H), spp=16, seed=0)       # first-hit feature buffers of render()'s camera samples
    f.albedo, f.normal, f.depth, f.coverage, f.instance               # views of f.data, (H, W, 16); albedo / roughness carry the graph
    clean = zdr_amd.denoise(image, f)                                 # edge-stopping filter guided by f, differentiable in the image
    clean = scene.render_denoised(material, res=(W, H), spp=16)       # the three calls in one

    E = torch.tensor([[0, 0, 0], [20, 20, 20]], dtype=torch.float32, device="cuda", requires_grad=True)   # one row per model
    image = scene.render(material, res=(W, H), spp=256, emissions=E)  # E.grad after backward(); the set of lights stays fixed

Images and materials are PyTorch tensors on the GPU; the renderer borrows their device pointers
for the duration of a call and enqueues its kernels on torch's current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np
import torch

from . import _native as N
from .geometry import SceneArrays, assemble, normalize_emission
from .mathtypes import Camera, float3, float4x4  # noqa: F401  (re-exported)

MAX_DEPTH = 16      # prb.py:15
RR_DEPTH = 2        # prb.py:16


def check_material_slots(slots, ninst: int) -> tuple:
    """A material slot table as ``Scene.material_slots`` takes it: one entry per model, an int in [0, MAX_MATERIALS) or None.
    Returns it as a tuple; raises ValueError otherwise."""
    if isinstance(slots, (str, bytes)) or not hasattr(slots, "__len__"):
        raise ValueError(f"material_slots must be a list with one entry per model, not {type(slots).__name__}")
    if len(slots) != ninst:
        raise ValueError(f"material_slots has {len(slots)} entries, the scene {ninst} models")
    out = []
    for i, k in enumerate(slots):
        if k is None:
            out.append(None)
            continue
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"material_slots[{i}] = {k!r}: a slot is an int or None")
        if not 0 <= int(k) < N.MAX_MATERIALS:
            raise ValueError(f"material_slots[{i}] = {k}: slots lie in [0, {N.MAX_MATERIALS})")
        out.append(int(k))
    return tuple(out)


def default_material_slots(emissions) -> tuple:
    """The slot table of a material list given without ``material_slots``: the k-th non-emitting model gets material k."""
    slots, k = [], 0
    for e in emissions:
        if (normalize_emission(e) > 0).any():
            slots.append(None)
        else:
            slots.append(k)
            k += 1
    return tuple(slots)


def resolve_material_slots(slots, emissions, nmat: int) -> tuple:
    """The slot table a call with ``nmat`` materials uses: ``slots`` (already checked), or the default one when it is None."""
    if not 1 <= nmat <= N.MAX_MATERIALS:
        raise ValueError(f"{nmat} materials given: between 1 and {N.MAX_MATERIALS} are supported")
    if slots is None:
        slots = default_material_slots(emissions)
        n = sum(k is not None for k in slots)
        if n != nmat:
            raise ValueError(f"{nmat} materials given for {n} non-emitting models: set material_slots, or pass one material per non-emitting model")
        return slots
    for i, k in enumerate(slots):
        if k is not None and k >= nmat:
            raise ValueError(f"material_slots[{i}] = {k}, but only {nmat} materials were given")
    return tuple(slots)


def check_emissions(emissions, ninst: int, device, envmap=None):
    """The tensor given as ``render(..., emissions=)`` / ``Scene.set_emission_values``: float32, (ninst, 3), on ``device``; not together
    with ``envmap=``.  Returns it; raises ValueError otherwise."""
    if envmap is not None:
        raise ValueError("emissions= and envmap= cannot be given in one call: differentiate the lights and the environment map in separate renders")
    if not isinstance(emissions, torch.Tensor) or emissions.dtype != torch.float32 or emissions.device != torch.device(device):
        raise ValueError(f"emissions must be a float32 tensor on {device}")
    if tuple(emissions.shape) != (ninst, 3):
        raise ValueError(f"emissions is {tuple(emissions.shape)}, the scene has {ninst} models: one (r, g, b) row per model, ({ninst}, 3)")
    return emissions


class EmissionValues(list):
    """``scene.emissions`` after ``set_emission_values``: the list that defines which models are lights (as given to ``Scene`` or
    ``update_lights``) with ``values``, the (ninst, 3) device tensor whose rows those lights now emit.  ``update_lights`` takes it back."""
    def __init__(self, base, values):
        super().__init__(base)
        self.values = values


class _ChannelViews:
    """``data``, an (H, W, 16) tensor, with each entry of the subclass's ``CHANNELS`` as an attribute: a view into it."""
    CHANNELS = {}

    def __init__(self, data):
        self.data = data

    def __getattr__(self, name):                       # (reached for names that are not attributes: the channels)
        if name not in self.CHANNELS:
            raise AttributeError(name)
        a, b = self.CHANNELS[name]
        return self.data[..., a] if b - a == 1 else self.data[..., a:b]


class Aovs(_ChannelViews):
    """First-hit feature buffers of ``Scene.render_aovs`` (include/zdr.h, zdr_render_aovs): ``data`` is the (H, W, 16) tensor, the
    attributes are views into it.  Every averaged channel is premultiplied by ``coverage`` (divide by it for the mean over the
    samples that hit); ``instance`` and ``slot`` are those of the pixel's first sample that hit, -1 where none did.  ``albedo`` and
    ``roughness`` are differentiable with respect to the materials; the views carry the graph."""
    CHANNELS = {"albedo": (0, 3), "roughness": (3, 4), "normal": (4, 7), "depth": (7, 8), "position": (8, 11), "coverage": (11, 12),
                "uv": (12, 14), "instance": (14, 15), "slot": (15, 16)}


class TexelAovs(_ChannelViews):
    """Texture-space feature buffers of ``Scene.texel_aovs`` (include/zdr.h, zdr_scene_texel_aovs): ``data`` is the (H, W, 16) tensor of
    one material's texels, the attributes are views into it.  ``coverage``: the texel's lattice point lies on a model; ``reach``: a
    bilinear lookup somewhere on a model can read the texel (so it can receive gradient); ``position``, ``normal``: of the surface at
    the texel, or at the closest point of the nearest triangle for a texel that is only reached; ``texel_size``: world length of one
    texel there; ``instance``, ``slot``: the model the texel belongs to and the material index, -1 where ``reach`` is 0.  The buffers
    depend on the geometry and the slot table only and carry no gradient.  The layout is ``Aovs``'s, so ``denoise`` takes them as guides.
    ``tangents``: the ``TexelTangents`` of the same texels when made with ``texel_aovs(..., tangents=True)``, else None."""
    CHANNELS = {"normal": (4, 7), "texel_size": (7, 8), "position": (8, 11), "coverage": (11, 12), "reach": (12, 13),
                "instance": (14, 15), "slot": (15, 16)}

    def __init__(self, data, tangents=None):
        super().__init__(data)
        self.tangents = tangents       # a TexelTangents from texel_aovs(..., tangents=True), else None

    def as_guides(self, reached=True):
        """A copy of ``data`` for ``denoise``, which reads channel 11 as its coverage: with ``reached`` that channel holds ``reach``, so
        that texels that are only reached take part in the normal and depth terms too — the form for seam padding."""
        g = self.data.clone()
        if reached:
            g[..., 11] = self.data[..., 12]
        return g

    def fill(self, x, by="coverage"):
        """``push_pull(x, self.coverage)``, or with ``by="reach"`` ``push_pull(x, self.reach)``: the (H, W, 4) texture ``x`` with every
        texel outside that mask filled from the ones inside it (zdr_amd/pushpull.py), differentiable in ``x``."""
        if by not in ("coverage", "reach"):
            raise ValueError(f'by must be "coverage" or "reach", not {by!r}')
        from .pushpull import push_pull
        return push_pull(x, getattr(self, by))


class TexelTangents:
    """The UV tangents of ``Scene.texel_aovs(..., tangents=True)`` (include/zdr.h, zdr_scene_texel_tangents): ``data`` is the (H, W, 8)
    tensor of one material's texels.  ``dpdx``, ``dpdy`` (H, W, 3): the world derivatives of the position per texture pixel to the right
    and DOWNWARDS (Y = (1 - v)(H - 1)); ``area`` (H, W): the world area of one texel, ``texel_size`` squared up to rounding;
    ``orientation`` (H, W): +1 or -1, the sign of (dpdx x dpdy) . normal — a mirrored chart has the other sign.  Eight zeros where
    the texel is not reached or ``texel_size`` is 0.  No gradient."""

    def __init__(self, data):
        self.data = data

    dpdx = property(lambda self: self.data[..., 0:3])
    area = property(lambda self: self.data[..., 3])
    dpdy = property(lambda self: self.data[..., 4:7])
    orientation = property(lambda self: self.data[..., 7])

    def metric(self):
        """The first fundamental form of the mapping per texel, (H, W, 3) = (dpdx . dpdx, dpdx . dpdy, dpdy . dpdy): what a
        metric-aware regulariser weighs texture differences with.  Torch code."""
        x, y = self.dpdx, self.dpdy
        return torch.stack([(x * x).sum(-1), (x * y).sum(-1), (y * y).sum(-1)], -1)


class TexelLighting:
    """Texture-space lighting of ``Scene.texel_lighting`` (include/zdr.h, zdr_scene_texel_lighting): ``data`` is the (H, W, 4) tensor of
    one material's texels, the shape of a material, so ``denoise`` filters it with ``TexelAovs.as_guides()``.  ``irradiance`` (H, W, 3):
    direct irradiance on the side the texel's normal points to; ``openness`` (H, W): the open fraction of the cosine-weighted hemisphere,
    up to ``max_distance``.  Four zeros where ``reach`` is 0.  ``irradiance`` carries a gradient in the emissions and the environment
    map when ``texel_lighting`` was given ``emissions=`` or ``envmap=``; ``openness`` never does."""

    def __init__(self, data):
        self.data = data

    @property
    def irradiance(self):
        return self.data[..., 0:3]

    @property
    def openness(self):
        return self.data[..., 3]


class TexelBounce:
    """Bounced light of ``Scene.texel_bounce`` (include/zdr.h, zdr_scene_texel_bounce): ``data`` is the (H, W, 4) tensor of one material's
    texels.  ``irradiance`` (H, W, 3): the irradiance that arrives after at least one Lambertian bounce, up to ``bounces`` of them;
    ``surface`` (H, W): the share of the cosine-weighted hemisphere that ends on the front of a model with a material — what can bounce
    light at all.  Four zeros where ``reach`` is 0.  ``irradiance`` carries a gradient in the materials that require grad and in the
    emissions when ``texel_bounce`` was given ``emissions=``; ``surface`` never does."""

    def __init__(self, data):
        self.data = data

    @property
    def irradiance(self):
        return self.data[..., 0:3]

    @property
    def surface(self):
        return self.data[..., 3]


class TexelView:
    """What a camera sees of each texel, from ``Scene.texel_view`` (include/zdr.h, zdr_scene_texel_view): ``data`` is the (H, W, 8) view
    buffer of one material's texels for an image of ``res`` = (width, height).  ``visible`` (H, W): 1 where the texel lies in front of the
    camera, inside its image and the segment to the camera is free; ``cosine``: n . wi towards the camera, signed (a weight, not a test);
    ``pixel`` (H, W, 2): the texel's position (X, Y) in the image, pixel x covering [x, x + 1); ``depth``, ``distance``: along the
    camera's axis and along the segment; ``scale``: the on-screen length of one texel in pixels.  Eight zeros where ``reach`` is 0.
    No gradient, unless the view was made from a camera tensor that requires grad (README, "Camera gradients"): then ``data`` carries
    gradient to it, ``visible`` held fixed.  ``footprint_data``: the (H, W, 4) footprint buffer (include/zdr.h, zdr_texel_footprint) when the view was made with
    ``footprint=True``, else None; ``footprint`` reads it.  ``footprint_patch``: what that buffer takes a texel to be — "square" (a
    square of side ``texel_size``), "uv" (the parallelogram of the texel's UV tangents) — or None without one."""

    def __init__(self, data, res, footprint_data=None, footprint_patch=None):
        self.data = data
        self.res = (int(res[0]), int(res[1]))
        self.footprint_data = footprint_data
        self.footprint_patch = footprint_patch if footprint_data is not None else None

    visible = property(lambda self: self.data[..., 0])
    cosine = property(lambda self: self.data[..., 1])
    pixel = property(lambda self: self.data[..., 2:4])
    depth = property(lambda self: self.data[..., 4])
    distance = property(lambda self: self.data[..., 5])
    scale = property(lambda self: self.data[..., 6])

    @property
    def footprint(self):
        """The on-screen ellipse of each texel, a ``TexelFootprint`` (``major_axis`` (H, W, 2), ``minor``, ``major``), or None when the
        view was made without ``footprint=True``."""
        return None if self.footprint_data is None else TexelFootprint(self.footprint_data)

    def gather(self, image, filter="bilinear", footprint=1.0, max_aniso=8, plan=None):
        """``texel_gather(image, self)`` (zdr_amd/project.py): the (height, width, 4) image of this view's size read into texture space,
        (H, W, 4), differentiable in ``image``.  ``filter``, ``footprint``, ``max_aniso``, ``plan``: as ``texel_gather`` takes them
        ("mip": prefiltered; "aniso": anisotropic, for a view made with ``footprint=True``; ``plan=True``: the gradient through a
        gather plan kept on this view, without float atomics)."""
        from .project import texel_gather
        if tuple(image.shape[:2]) != (self.res[1], self.res[0]):
            raise ValueError(f"the image must be ({self.res[1]}, {self.res[0]}, 4), the size the view was made for, not {tuple(image.shape)}")
        if plan is not None:
            return texel_gather(image, self, filter=filter, footprint=footprint, max_aniso=max_aniso, plan=plan)
        if filter == "aniso":
            return texel_gather(image, self, filter=filter, footprint=footprint, max_aniso=max_aniso)
        return texel_gather(image, self.data, filter=filter, footprint=footprint)

    def gather_plan(self, res=None, filter="bilinear", footprint=1.0, max_aniso=8, levels=0):
        """``zdr_amd.gather_plan(self, res, ...)`` (zdr_amd/plan.py): the ``GatherPlan`` of this view for images of ``res`` (default: the
        size the view was made for) — the adjoint of ``gather`` as CSR rows, built once (ONE synchronisation) and applied without
        float atomics."""
        from .plan import gather_plan
        return gather_plan(self, self.res if res is None else res, filter, footprint, max_aniso, levels)

    def weight(self, cosine_power=1.0):
        """``visible * |cosine| ** cosine_power`` (H, W): how much this view should count for each texel."""
        return self.visible * self.cosine.abs() ** float(cosine_power)


class TexelFootprint:
    """The footprint buffer of a view (include/zdr.h, zdr_texel_footprint), ``data`` (H, W, 4): the on-screen ellipse of each texel's
    patch (square, or with ``footprint="uv"`` the parallelogram of its UV tangents).  ``major_axis`` (H, W, 2): the long axis as a vector in pixels; ``minor``, ``major`` (H, W): the lengths of the two
    axes (``major`` = |``major_axis``|).  Zeros where the texel is not shaded or lies behind the camera.  No gradient."""

    def __init__(self, data):
        self.data = data

    major_axis = property(lambda self: self.data[..., 0:2])
    minor = property(lambda self: self.data[..., 2])
    major = property(lambda self: self.data[..., 3])


class TexelProjection:
    """Several photographs merged in texture space, from ``Scene.texel_project``: ``color`` (H, W, 4) = sum w_i c_i / sum w_i (0 where no
    view sees the texel), ``weight`` (H, W) = sum w_i, ``count`` (H, W): the number of views that see each texel."""

    def __init__(self, color, weight, count):
        self.color, self.weight, self.count = color, weight, count


def _camera_pod(cam: Camera) -> N.CameraPOD:
    return N.CameraPOD(float(cam.fov), (C.c_float * 3)(*cam.origin), (C.c_float * 3)(*cam.target), (C.c_float * 3)(*cam.up))


def _camera_arg(camera, default):
    """``camera`` of the texel-view calls -> (Camera, the camera tensor or None).  A tensor is a differentiable camera: 10 float32
    values on the CPU in ``Camera.to_tensor``'s order, read on the host — float32 to float32, so the bits are those of the ``Camera``."""
    if not isinstance(camera, torch.Tensor):
        return (camera if camera is not None else default), None
    if camera.device.type != "cpu":
        raise ValueError(f"a camera tensor must be on the CPU (it is read on the host), not on {camera.device}")
    if camera.dtype != torch.float32 or camera.numel() != 10:
        raise ValueError(f"a camera tensor is 10 float32 values (fov, origin, target, up), not {tuple(camera.shape)} {camera.dtype}")
    return Camera.from_tensor(camera), camera


class TexelViewOperator(torch.autograd.Function):
    """view.data = texel_view(camera tensor): the forward is ``Scene.texel_view_forward`` with the tensor's values, the backward
    ``Scene.texel_view_backward`` (visibility held fixed) and a copy of its 10 floats to the host — ONE synchronisation per backward."""
    @staticmethod
    def forward(ctx, camera, texel_data, scene, res):
        ctx.scene, ctx.res, ctx.camera, ctx.shape = scene, res, Camera.from_tensor(camera), camera.shape
        ctx.save_for_backward(texel_data)
        return scene.texel_view_forward(texel_data, res, camera=ctx.camera)

    @staticmethod
    def backward(ctx, grad_output):
        texel_data, = ctx.saved_tensors
        d = ctx.scene.texel_view_backward(texel_data, grad_output.contiguous(), ctx.res, camera=ctx.camera)
        return d.cpu().reshape(ctx.shape), None, None, None


class Scene:
    """A 3D scene for differentiable rendering w.r.t. (H, W, 4) material textures
    (diffuse rgb + roughness; specular fixed at 0.04).  With one material tensor only the first model is
    textured; any other model is a light (emission > 0) or a blocker (render.py:31-71, prb.py:45).  With a
    list of materials each model is shaded by the material ``material_slots`` gives it (see ``render``).

    Attributes:
        camera (Camera): fov (full horizontal angle, radians), origin, target, up.
        use_tent_filter (bool): tent reconstruction filter if True (default), box filter if False.
        sampler (str): "cmj" (correlated multi-jitter, corrmj.py — default here) or "pmj02bn"
            (needs tables, see ``set_pmj02bn_tables``; the reference's tables are not shipped).
        material_slots (list | None): one entry per model, the index of its material in the list given to
            ``render`` or None (path / direct: a light or a blocker as without materials; collocated: black).
            None (default): a single material tensor shades model 0 as the reference does, and a list shades
            the k-th non-emitting model with its k-th material.
    """

    def __init__(self, models, integrator="direct", *, device=None, accel="auto", sampler="cmj"):
        integrators = {"path": N.PATH, "direct": N.DIRECT, "collocated": N.COLLOCATED}
        self._integrator = integrators[integrator]          # KeyError on unknown names, as render.py:70
        self.integrator = integrator
        if not torch.cuda.is_available():
            raise N.ZdrError("zdr_amd needs an AMD GPU (HIP device); there is no CPU back end")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else torch.device(device).index or 0)
        self.camera = Camera(fov=40 / 180 * 3.1415926, origin=float3(1.0, 0.5, 0.0), target=float3(0.0, 0.0, 0.0), up=float3(0.0, 1.0, 0.0))
        self.use_tent_filter = True
        self.sampler = sampler
        self.max_depth = MAX_DEPTH
        self.rr_depth = RR_DEPTH
        self.prb_mode = "expectation"      # or "detached": the reference's constant-roulette / constant-MIS adjoint; "literal": with the BSDF-sample seed of prb.py:162 as written (include/zdr.h)
        self.env_count = 0
        self._env_compensate_mis = True    # what the environment map's tables were last built with (add_envmap, update_envmap_sampling)
        self._handle = None
        self._material_slots = None
        self._uploaded_slots = None        # the slot table the native scene holds (None: never uploaded)
        self.load_geometry(models, accel=accel)

    # ------------------------------------------------------------------ geometry / lights
    def load_geometry(self, models, accel="auto"):
        arrays = models if isinstance(models, SceneArrays) else assemble(models)
        self._arrays = arrays
        self.inst_count = arrays.ninst
        self.emissions = [float3(*e) for e in arrays.inst_emission.tolist()]
        self.light_count = int((arrays.inst_emission > 0).any(axis=1).sum())
        h = C.c_void_p()
        L = N.lib()
        if getattr(self, "_finalizer", None) is not None:   # a second load_geometry: the old handle (and the tables set on it) go
            self._finalizer()
            self._handle, self.env_count, self._pmj_tables_set = None, 0, False
        self._material_slots = None
        self._uploaded_slots = None
        N.check(L.zdr_scene_create(arrays.verts.ctypes.data, arrays.verts.shape[0], arrays.tris.ctypes.data, arrays.tris.shape[0],
                                   arrays.inst_tri_begin.ctypes.data, arrays.inst_xform.ctypes.data, arrays.inst_emission.ctypes.data,
                                   arrays.ninst, self.device.index, N.ACCELS[accel], C.byref(h)))
        self._handle = h
        self._finalizer = weakref.finalize(self, L.zdr_scene_destroy, h)

    def info(self) -> dict:
        i = N.SceneInfo()
        N.check(N.lib().zdr_scene_info(self._handle, C.byref(i)))
        d = {k: getattr(i, k) for k, _ in N.SceneInfo._fields_}
        d["accel"] = {N.ACCEL_BRUTE: "brute", N.ACCEL_BVH: "bvh"}[i.accel]
        return d

    def update_lights(self, emissions):
        """Rewrite the emission of each mesh in the scene (light-stage style switching);
        ``emissions`` has one entry per model: None, a number or a float3 (render.py:130-148)."""
        assert len(emissions) == self.inst_count
        self.emissions = emissions
        e = np.ascontiguousarray(np.stack([normalize_emission(x) for x in emissions]), np.float32)
        self.light_count = int((e > 0).any(axis=1).sum())
        N.check(N.lib().zdr_scene_set_emissions(self._handle, e.ctypes.data, self._stream()))
        if isinstance(emissions, EmissionValues):         # a snapshot of set_emission_values: the light list, then its values
            self._apply_emission_values(emissions.values)

    def set_emission_values(self, emissions):
        """Rewrites, in place and without a synchronise, the emission of the models that are lights now (include/zdr.h,
        zdr_scene_set_emission_values): ``emissions`` is a float32 (ninst, 3) tensor on the scene's device; rows of models outside the
        light list of ``Scene(...)`` or of the last ``update_lights`` are ignored.  The values stay the scene's emissions until the next
        call or ``update_lights``."""
        values = check_emissions(emissions, self.inst_count, self.device).detach().contiguous()
        self._apply_emission_values(values)
        self.emissions = EmissionValues(self.emissions, values)   # a new object: the autograd nodes compare identities

    def _apply_emission_values(self, values):
        N.check(N.lib().zdr_scene_set_emission_values(self._handle, values.data_ptr(), self._stream()))

    def _check_d_emission(self, d_emission, d_env):
        if d_env is not None:
            raise ValueError("d_emission and d_env cannot be given in one call")
        if (tuple(d_emission.shape) != (self.inst_count, 3) or not d_emission.is_contiguous() or d_emission.device != self.device
                or d_emission.dtype != torch.float32):
            raise ValueError(f"d_emission must be a contiguous float32 ({self.inst_count}, 3) tensor on {self.device}")

    def add_envmap(self, image, compensate_mis=True):
        """Adds a lat-long environment light (render.py:150-156, envmap.py:116-203).  ``image`` is an
        (H, W, 3|4) float array / tensor (2:1 or 1:1) or the path of an OpenEXR file (the reference reads it
        through imageio; here zdr_amd/exr.py: scan-line files, NONE / RLE / ZIPS / ZIP / PIZ compression) or of a ``.npy``
        file.  ``None`` removes it."""
        from . import envmap as E
        if image is None:
            N.check(N.lib().zdr_scene_set_envmap(self._handle, None, 0, 0, None, None, None, 0, 0))
            self.env_count = 0
            return
        if isinstance(image, str):
            image = E.load_image(image)               # .exr (zdr_amd/exr.py) or .npy
        if isinstance(image, torch.Tensor):
            image = image.detach().cpu().numpy()
        img = E.prepare_image(image)
        prob, alias, pdf = E.build_tables(img, compensate_mis=compensate_mis)
        N.check(N.lib().zdr_scene_set_envmap(self._handle, img.ctypes.data, img.shape[0], img.shape[1], prob.ctypes.data, alias.ctypes.data,
                                             pdf.ctypes.data, E.SAMPLE_MAP_W, E.SAMPLE_MAP_H))
        self.env_count = 1
        self._envmap = (img, prob, alias, pdf)        # kept for tests / the oracle
        self._env_compensate_mis = bool(compensate_mis)

    def update_envmap_sampling(self, image, compensate_mis=True, on_device=False):
        """Rebuilds the environment map's importance-sampling tables from ``image`` (and uploads it as the map): ``add_envmap`` for
        a map that is being optimised.  ``render(..., envmap=)`` keeps the tables of the last ``add_envmap`` or of this call, and
        differentiates with them held fixed.  Like ``add_envmap`` this synchronises the device and replaces the scene's buffers,
        so graphs captured before no longer see the map.

        ``on_device=True`` rebuilds them on the GPU instead (include/zdr.h, zdr_scene_update_envmap_sampling): ``image`` is a float32
        tensor on the scene's device, of add_envmap's size as ``render(..., envmap=)`` takes it, or None for the map the scene holds.
        It is uploaded in place (set_envmap_texture) and the tables are rebuilt in the scene's buffers, on torch's current stream:
        no copy to the host, no synchronisation, no new buffers, so the call can be captured in a graph once it has been made once,
        and graphs captured earlier read the new tables.  The host copies of the tables in ``_envmap[1:]`` are then stale until
        ``envmap_sampling_tables()`` refreshes them."""
        if on_device:
            if self.env_count == 0:
                raise ValueError("the scene has no environment map: call add_envmap first")
            if image is not None:
                self.set_envmap_texture(self._prepare_envmap(image))
            N.check(N.lib().zdr_scene_update_envmap_sampling(self._handle, 1 if compensate_mis else 0, self._stream()))
            self._env_compensate_mis = bool(compensate_mis)
            return
        if image is None:
            raise ValueError("update_envmap_sampling needs a map (add_envmap(None) removes it)")
        self.add_envmap(image.detach() if isinstance(image, torch.Tensor) else image, compensate_mis=compensate_mis)

    def envmap_sampling_tables(self):
        """(alias_prob, alias_idx, pdf) as the device holds them now, as NumPy arrays in add_envmap's layout (the marginal table first,
        then the rows); synchronises torch's current stream.  Also refreshes the host copies in ``_envmap[1:]``, which an on-device
        rebuild leaves behind."""
        from . import envmap as E
        if self.env_count == 0:
            raise ValueError("the scene has no environment map: call add_envmap first")
        n = E.SAMPLE_MAP_H + E.SAMPLE_MAP_H * E.SAMPLE_MAP_W
        prob, alias, pdf = np.empty(n, np.float32), np.empty(n, np.int32), np.empty(E.SAMPLE_MAP_H * E.SAMPLE_MAP_W, np.float32)
        N.check(N.lib().zdr_scene_get_envmap_sampling(self._handle, prob.ctypes.data, alias.ctypes.data, pdf.ctypes.data, self._stream()))
        self._envmap = (self._envmap[0], prob, alias, pdf)
        return prob, alias, pdf

    def _prepare_envmap(self, envmap):
        """The tensor given as ``render(..., envmap=)``, prepared in torch (envmap.prepare_tensor) so that autograd returns its
        gradient in the caller's shape; its size must be the one given to add_envmap."""
        from . import envmap as E
        if self.env_count == 0:
            raise ValueError("envmap= needs an environment map: call add_envmap first (it builds the importance-sampling tables)")
        if not isinstance(envmap, torch.Tensor) or envmap.device != self.device or envmap.dtype != torch.float32:
            raise ValueError(f"envmap must be a float32 tensor on {self.device}")
        try:
            env = E.prepare_tensor(envmap)
        except RuntimeError as e:
            raise ValueError(str(e)) from None
        if tuple(env.shape) != tuple(self._envmap[0].shape):
            raise ValueError(f"envmap {tuple(envmap.shape)} is {tuple(env.shape)} once prepared, the scene's map {tuple(self._envmap[0].shape)}: "
                             "the size must stay that of add_envmap")
        return env

    def set_envmap_texture(self, env):
        """Replaces the environment map's texels in place (include/zdr.h, zdr_scene_set_envmap_texture): ``env`` is the prepared
        (H, H, 4) float32 map on the scene's device, of add_envmap's size.  The importance-sampling tables are kept."""
        if self.env_count == 0:
            raise ValueError("the scene has no environment map: call add_envmap first")
        if tuple(env.shape) != tuple(self._envmap[0].shape) or env.device != self.device or env.dtype != torch.float32:
            raise ValueError(f"env must be a float32 {tuple(self._envmap[0].shape)} tensor on {self.device}")
        env = env.detach().contiguous()
        if env.data_ptr() % 16:                             # the copy moves float4 texels: a view at an odd offset is copied first
            env = env.clone()
        N.check(N.lib().zdr_scene_set_envmap_texture(self._handle, env.data_ptr(), self._stream()))

    def _check_d_env(self, d_env):
        if self.env_count == 0:
            raise ValueError("d_env needs an environment map: call add_envmap first")
        if tuple(d_env.shape) != tuple(self._envmap[0].shape) or not d_env.is_contiguous() or d_env.device != self.device or d_env.dtype != torch.float32:
            raise ValueError(f"d_env must be a contiguous float32 {tuple(self._envmap[0].shape)} tensor on {self.device}")

    def set_pmj02bn_tables(self, pmj_samples, blue_noise):
        """pmj_samples: uint32 [nsets][nsamples][2]; blue_noise: uint16 [ntex][res][res] (pmj02bn.py:9-18)."""
        pmj = np.ascontiguousarray(pmj_samples, np.uint32)
        bn = np.ascontiguousarray(blue_noise, np.uint16)
        assert pmj.ndim == 3 and pmj.shape[2] == 2 and bn.ndim == 3 and bn.shape[1] == bn.shape[2]
        N.check(N.lib().zdr_scene_set_pmj02bn_tables(self._handle, pmj.ctypes.data, pmj.shape[0], pmj.shape[1], bn.ctypes.data, bn.shape[0], bn.shape[1]))
        self._pmj_tables_set = True

    def _ensure_pmj_tables(self):
        """The reference's pbrt tables are not shipped: without tables of the caller's, generated ones (zdr_amd/pmj02bn_tables.py)."""
        if not getattr(self, "_pmj_tables_set", False):
            from . import pmj02bn_tables
            self.set_pmj02bn_tables(*pmj02bn_tables.default_tables(verbose=True))

    # -------------------------------------------------------------------------- materials
    @property
    def material_slots(self):
        return None if self._material_slots is None else list(self._material_slots)

    @material_slots.setter
    def material_slots(self, slots):
        if slots is None:
            self._material_slots = None
            return
        slots = check_material_slots(slots, self.inst_count)
        self._upload_slots(slots)
        self._material_slots = slots

    def _upload_slots(self, slots: tuple):
        if slots == self._uploaded_slots:
            return
        table = np.array([-1 if k is None else k for k in slots], np.int32)
        N.check(N.lib().zdr_scene_set_material_slots(self._handle, table.ctypes.data, self._stream()))
        self._uploaded_slots = slots

    def _call_slots(self, nmat, model0=False):
        """The slot table of a call with ``nmat`` materials: ``material_slots``, or the default mapping — or, ``model0`` and
        ``material_slots`` unset, material 0 on model 0 alone."""
        if model0 and self._material_slots is None:
            return (0,) + (None,) * (self.inst_count - 1)
        return resolve_material_slots(self._material_slots, self.emissions, nmat)

    def _resolve_materials(self, material, single_is_model0=False, pack=True):
        """(mats, slots, dims, packed) of ``material`` as ``render`` takes it, a tensor or a list of tensors: the list, the slot table
        that goes with it, the sizes, and (``pack``; else None) the texels as one tensor, which carries the graph: a copy when there
        are several.  ``single_is_model0``: with ``material_slots`` unset a single tensor belongs to model 0 alone."""
        mats = list(material) if isinstance(material, (list, tuple)) else [material]
        for m in mats:
            self._check_material(m)
        slots = self._call_slots(len(mats), single_is_model0 and not isinstance(material, (list, tuple)))
        dims = tuple((int(m.shape[0]), int(m.shape[1])) for m in mats)
        packed = None if not pack else mats[0] if len(mats) == 1 else torch.cat([m.reshape(-1, 4) for m in mats])
        return mats, slots, dims, packed

    def _material_call(self, materials, dims, slots=None):
        """(packed material tensor, int32 dims array, slot table) of a material-table call: ``materials`` is a list / tuple of
        (H, W, 4) tensors (packed here, a copy when there are several), or one packed tensor with ``dims`` = [(h, w), ...]."""
        if isinstance(materials, (list, tuple)):
            mats = list(materials)
            for m in mats:
                self._check_material(m)
            dims = [(int(m.shape[0]), int(m.shape[1])) for m in mats]
            packed = mats[0].detach().contiguous() if len(mats) == 1 else torch.cat([m.detach().reshape(-1, 4) for m in mats])
        else:
            if dims is None:
                raise ValueError("a packed material tensor needs dims = [(h, w), ...]")
            packed = materials.detach().contiguous()
            if packed.device != self.device or packed.dtype != torch.float32:
                raise ValueError(f"materials must be float32 tensors on {self.device}")
            dims = [(int(h), int(w)) for h, w in dims]
            if packed.numel() != 4 * sum(h * w for h, w in dims):
                raise ValueError(f"the packed materials hold {packed.numel() // 4} texels, dims {sum(h * w for h, w in dims)}")
        if slots is None:
            slots = resolve_material_slots(self._material_slots, self.emissions, len(dims))
        self._upload_slots(tuple(slots))
        return packed, np.ascontiguousarray(np.array(dims, np.int32).reshape(-1, 2)), tuple(slots)

    def _pack_grads(self, d_materials, packed):
        """``d_materials`` — a list shaped like the materials, or one tensor — as the one tensor a native backward accumulates into:
        a copy when the list holds several, which _unpack_grads copies back."""
        listed = isinstance(d_materials, (list, tuple))
        dpacked = (torch.cat([g.reshape(-1, 4) for g in d_materials]) if len(d_materials) > 1 else d_materials[0]) if listed else d_materials
        if dpacked.numel() != packed.numel() or not dpacked.is_contiguous() or dpacked.device != self.device or dpacked.dtype != torch.float32:
            raise ValueError(f"d_materials must be contiguous float32 on {self.device}, shaped like the materials")
        return dpacked

    @staticmethod
    def _unpack_grads(dpacked, d_materials):
        if isinstance(d_materials, (list, tuple)) and len(d_materials) > 1:
            off = 0
            for t in d_materials:
                t.copy_(dpacked[off:off + t.numel() // 4].reshape(t.shape))
                off += t.numel() // 4
        return d_materials

    def render_forward_materials(self, materials, res, spp, seed, *, dims=None, rect=None, samples=None, out=None, tile_shard=None, slots=None):
        """``render_forward`` with one material per slot (include/zdr.h, zdr_render_forward_materials).  ``materials``: a list of
        (H_k, W_k, 4) tensors, or their packed texels with ``dims``.  ``slots``: the slot table to use (default: ``material_slots``,
        or the default mapping)."""
        packed, d, _ = self._material_call(materials, dims, slots)
        image = self._image_out(out, res)
        p = self._params(res, spp, seed, (1, 1), rect, samples, tile_shard=tile_shard)
        N.check(N.lib().zdr_render_forward_materials(self._handle, C.byref(p), packed.data_ptr(), d.ctypes.data, d.shape[0], image.data_ptr(), self._stream()))
        return image

    def render_backward_materials(self, grad_output, d_materials, materials, res, spp, seed, *, dims=None, rect=None, samples=None, camera=None,
                                  tile_shard=None, slots=None, d_env=None, d_emission=None):
        """``render_backward`` with one material per slot: accumulates into ``d_materials`` (a list shaped like ``materials``, or
        one packed tensor); uses ``seed + 1`` like render_backward.  ``d_env``, ``d_emission``: as in render_backward."""
        packed, d, _ = self._material_call(materials, dims, slots)
        dpacked = self._pack_grads(d_materials, packed)
        g = grad_output.reshape(res[1], res[0], 4).to(device=self.device, dtype=torch.float32).contiguous()
        p = self._params(res, spp, seed + 1, (1, 1), rect, samples, camera, tile_shard=tile_shard)
        self._native_backward(p, g, packed, d, dpacked, d_env, d_emission)
        return self._unpack_grads(dpacked, d_materials)

    # --------------------------------------------------------------------- feature buffers
    def _aov_call(self, materials, dims, slots):
        """_material_call for the feature buffers: one (H, W, 4) tensor is a list of one, and without ``slots`` and ``material_slots``
        one material belongs to model 0 alone — what the path and the direct integrator do with a single material."""
        if isinstance(materials, torch.Tensor) and dims is None:
            materials = [materials]
        if slots is None and (len(dims) if dims is not None else len(materials)) == 1:
            slots = self._call_slots(1, model0=True)
        return self._material_call(materials, dims, slots)

    def render_aovs_forward(self, materials, res, spp, seed, *, dims=None, slots=None, rect=None, tile_shard=None, out=None):
        """The (H, W, 16) feature buffers of include/zdr.h, zdr_render_aovs, rendered with the camera samples of ``render_forward``
        of the same ``seed``.  ``materials``, ``dims``, ``slots``: as ``render_forward_materials`` (one tensor: a list of one, on model
        0 unless ``material_slots`` says otherwise).  With ``rect`` / ``tile_shard`` only that shard is written; other pixels of
        ``out`` keep their value, a fresh buffer is zero-filled."""
        packed, d, _ = self._aov_call(materials, dims, slots)
        out = self._out_tensor(out, (int(res[1]), int(res[0]), N.AOV_CHANNELS), True)
        p = self._params(res, spp, seed, (1, 1), rect, None, tile_shard=tile_shard)
        N.check(N.lib().zdr_render_aovs(self._handle, C.byref(p), packed.data_ptr(), d.ctypes.data, d.shape[0], out.data_ptr(), self._stream()))
        return out

    def render_aovs_backward(self, grad, d_materials, materials, res, spp, seed, *, dims=None, slots=None, camera=None, rect=None, tile_shard=None):
        """The adjoint of ``render_aovs_forward`` with respect to the materials: accumulates into ``d_materials`` (a list shaped
        like ``materials``, one tensor, or the packed texels).  ``grad`` is the (H, W, 16) cotangent, of which floats 0..3 are read.
        The SAME ``seed`` as the forward: this is its exact transpose."""
        packed, d, _ = self._aov_call(materials, dims, slots)
        dpacked = self._pack_grads(d_materials, packed)
        g = grad.reshape(res[1], res[0], N.AOV_CHANNELS).to(device=self.device, dtype=torch.float32).contiguous()
        p = self._params(res, spp, seed, (1, 1), rect, None, camera, tile_shard=tile_shard)
        N.check(N.lib().zdr_render_aovs_backward(self._handle, C.byref(p), g.data_ptr(), packed.data_ptr(), d.ctypes.data, d.shape[0],
                                                 dpacked.data_ptr(), self._stream()))
        return self._unpack_grads(dpacked, d_materials)

    class AovOperator(torch.autograd.Function):
        """render_aovs() of the packed texels of its materials: returns the (H, W, 16) buffers and, backward, the packed gradient
        (torch.cat's own backward hands each material its part).  The camera is snapshotted like RenderOperator's."""
        @staticmethod
        def forward(ctx, packed, self, res, spp, seed, dims, slots):
            ctx.save_for_backward(packed)
            ctx.scene = weakref.ref(self)
            ctx.args = (res, spp, seed, dims, slots)
            ctx.camera = self.camera.copy()
            return self.render_aovs_forward(packed, res, spp, seed, dims=dims, slots=slots)

        @staticmethod
        def backward(ctx, grad_output):
            scene = ctx.scene()
            packed, = ctx.saved_tensors
            res, spp, seed, dims, slots = ctx.args
            grad = torch.zeros(packed.size(), dtype=packed.dtype, device=packed.device)
            scene.render_aovs_backward(grad_output, grad, packed.detach(), res, spp, seed, dims=dims, slots=slots, camera=ctx.camera)
            return grad, None, None, None, None, None, None

    def render_aovs(self, material, *, res, spp, seed=0) -> Aovs:
        """What each pixel sees: an ``Aovs`` whose ``data`` is the (height, width, 16) tensor of include/zdr.h, zdr_render_aovs —
        albedo, roughness, normal, depth, position, coverage, uv, instance and slot of the first hit, averaged over the camera
        samples that ``render(material, res=res, spp=spp, seed=seed)`` draws — with a named view for each.  ``material`` is a tensor
        or a list exactly as ``render`` takes it; albedo and roughness are differentiable with respect to it (to each tensor of a
        list).  The scene's integrator does not matter.  With one tensor and ``material_slots`` unset only model 0 has a material
        (slot 0), as in the path and direct integrators; every other model reads albedo 0 and slot -1."""
        _, slots, dims, packed = self._resolve_materials(material, True)
        return Aovs(Scene.AovOperator.apply(packed, self, res, spp, seed, dims, slots))

    # ------------------------------------------------------------- texture-space buffers
    def texel_aovs_forward(self, index, tex_hw, *, slots=None, out=None, workspace=None):
        """The (H, W, 16) texture-space buffers of include/zdr.h, zdr_scene_texel_aovs, for material ``index`` at ``tex_hw`` = (H, W).
        ``slots``: the slot table to use (default: the one the scene holds).  ``out`` and ``workspace`` (any tensor of at least
        ``zdr_texel_aovs_workspace_bytes`` bytes) are allocated when not given.  Only enqueues, on torch's current stream."""
        H, W = int(tex_hw[0]), int(tex_hw[1])
        if slots is not None:
            self._upload_slots(check_material_slots(slots, self.inst_count))
        workspace = self._workspace(workspace, int(N.lib().zdr_texel_aovs_workspace_bytes(H, W)))
        out = self._out_tensor(out, (H, W, N.AOV_CHANNELS), False)
        N.check(N.lib().zdr_scene_texel_aovs(self._handle, int(index), H, W, out.data_ptr(), workspace.data_ptr(), self._stream()))
        return out

    def texel_tangents_forward(self, index, tex_hw, *, slots=None, out=None, aovs_out=None, workspace=None):
        """zdr_scene_texel_tangents: ``(aovs, tangents)``, the (H, W, 16) buffers of ``texel_aovs_forward`` — the same bits — and the
        (H, W, 8) UV tangents (include/zdr.h) of material ``index`` at ``tex_hw`` = (H, W), in one call: the raster runs once.
        ``slots``: as ``texel_aovs_forward``.  ``out`` (the tangents), ``aovs_out`` and ``workspace`` (any tensor of at least
        ``zdr_texel_aovs_workspace_bytes`` bytes) are allocated when not given.  Only enqueues, on torch's current stream."""
        H, W = int(tex_hw[0]), int(tex_hw[1])
        if slots is not None:
            self._upload_slots(check_material_slots(slots, self.inst_count))
        workspace = self._workspace(workspace, int(N.lib().zdr_texel_aovs_workspace_bytes(H, W)))
        aovs_out = self._out_tensor(aovs_out, (H, W, N.AOV_CHANNELS), False)
        out = self._out_tensor(out, (H, W, 8), False)
        N.check(N.lib().zdr_scene_texel_tangents(self._handle, int(index), H, W, aovs_out.data_ptr(), out.data_ptr(), workspace.data_ptr(), self._stream()))
        return aovs_out, out

    def texel_aovs(self, material, index=0, tangents=False) -> TexelAovs:
        """What each texel of ``material[index]`` is: a ``TexelAovs`` whose ``data`` is the (H, W, 16) tensor of include/zdr.h,
        zdr_scene_texel_aovs, at that material's size — coverage, reach, world position, normal, texel size, instance and slot, with a
        named view for each.  ``material`` is a tensor or a list exactly as ``render_aovs`` takes it; it is used for its sizes and to
        resolve the slots only (with one tensor and ``material_slots`` unset only model 0 has material 0).  ``tangents=True``: one
        call of ``texel_tangents_forward`` instead, and ``.tangents`` is the ``TexelTangents`` of the same texels (README, "UV
        tangents"); without it ``.tangents`` is None.  No gradient."""
        _, slots, dims, _ = self._resolve_materials(material, True, pack=False)
        if not 0 <= int(index) < len(dims):
            raise ValueError(f"index {index}: {len(dims)} materials were given")
        if tangents:
            data, tan = self.texel_tangents_forward(int(index), dims[int(index)], slots=slots)
            return TexelAovs(data, TexelTangents(tan))
        return TexelAovs(self.texel_aovs_forward(int(index), dims[int(index)], slots=slots))

    # ------------------------------------------------------------- texture-space lighting
    def texel_lighting_forward(self, texel_data, *, spp, seed=0, samples=None, max_distance=None, sampler=None, out=None, workspace=None):
        """The (H, W, 4) lighting buffer of include/zdr.h, zdr_scene_texel_lighting — direct irradiance (floats 0..2) and openness
        (float 3) — for the surface points of ``texel_data``, an (H, W, 16) tensor in the layout of ``texel_aovs_forward`` of which the
        normal, the position and ``reach`` are read.  ``samples`` = (begin, end): a subrange of [0, spp) (default: all; the outputs of
        disjoint ranges add up).  ``max_distance``: how far an openness ray looks (default 1e30: sky visibility; finite: ambient
        occlusion).  ``sampler``: "cmj" or "pmj02bn" (default: the scene's).  ``out`` and ``workspace`` (any tensor of at least
        ``zdr_texel_lighting_workspace_bytes`` bytes) are allocated when not given.  Only enqueues, on torch's current stream."""
        if texel_data.ndim != 3 or texel_data.shape[2] != N.AOV_CHANNELS or texel_data.dtype != torch.float32 or texel_data.device != self.device:
            raise ValueError(f"texel_data must be a float32 (H, W, {N.AOV_CHANNELS}) tensor on {self.device}")
        texel_data = texel_data.detach().contiguous()
        H, W = int(texel_data.shape[0]), int(texel_data.shape[1])
        sampler = self.sampler if sampler is None else sampler
        if sampler not in N.SAMPLERS:
            raise ValueError(f"unknown sampler {sampler!r}")
        if sampler == "pmj02bn":
            self._ensure_pmj_tables()
        workspace = self._workspace(workspace, int(N.lib().zdr_texel_lighting_workspace_bytes(H, W)))
        out = self._out_tensor(out, (H, W, 4), False)
        p = N.TexelLightingParams()
        p.struct_size = C.sizeof(N.TexelLightingParams)
        p.tex_h, p.tex_w, p.spp, p.seed, p.sampler = H, W, int(spp), int(seed) & 0xFFFFFFFF, N.SAMPLERS[sampler]
        begin, end = (0, int(spp)) if samples is None else (int(samples[0]), int(samples[1]))
        if not 0 <= begin < end <= int(spp):
            raise ValueError(f"samples {(begin, end)} must be a non-empty subrange of [0, {int(spp)})")
        p.sample_begin, p.sample_end = begin, end
        p.max_distance = 1e30 if max_distance is None else float(max_distance)
        N.check(N.lib().zdr_scene_texel_lighting(self._handle, C.byref(p), texel_data.data_ptr(), out.data_ptr(), workspace.data_ptr(), self._stream()))
        return out

    def texel_lighting_backward(self, texel_data, d_out, *, spp, seed=0, samples=None, sampler=None, d_emission=None, d_env=None, workspace=None):
        """The adjoint of ``texel_lighting_forward``'s irradiance (include/zdr.h, zdr_scene_texel_lighting_backward): with the cotangent
        ``d_out`` (H, W, 4) — float 3, the openness', is ignored — ADDS the gradient of the lights' emissions into ``d_emission``, a
        float32 (ninst, 3) tensor, and that of the environment map into ``d_env``, a prepared float32 tensor of the map's size; one of
        the two at least, both in one call are allowed.  ``spp``, ``seed``, ``samples`` and ``sampler`` are the forward's (the same
        seed), and the scene must hold the forward's emissions and map: the acceptance test is replayed with them.  Not bit-stable
        from run to run (float atomics).  Only enqueues, on torch's current stream.  Returns (d_emission, d_env)."""
        if texel_data.ndim != 3 or texel_data.shape[2] != N.AOV_CHANNELS or texel_data.dtype != torch.float32 or texel_data.device != self.device:
            raise ValueError(f"texel_data must be a float32 (H, W, {N.AOV_CHANNELS}) tensor on {self.device}")
        texel_data = texel_data.detach().contiguous()
        H, W = int(texel_data.shape[0]), int(texel_data.shape[1])
        if not isinstance(d_out, torch.Tensor) or tuple(d_out.shape) != (H, W, 4) or d_out.dtype != torch.float32 or d_out.device != self.device:
            raise ValueError(f"d_out must be a float32 ({H}, {W}, 4) tensor on {self.device}")
        d_out = d_out.detach().contiguous()
        if d_emission is None and d_env is None:
            raise ValueError("texel_lighting_backward needs d_emission, d_env or both")
        if d_emission is not None:
            self._check_d_emission(d_emission, None)
        if d_env is not None:
            self._check_d_env(d_env)
        sampler = self.sampler if sampler is None else sampler
        if sampler not in N.SAMPLERS:
            raise ValueError(f"unknown sampler {sampler!r}")
        if sampler == "pmj02bn":
            self._ensure_pmj_tables()
        begin, end = (0, int(spp)) if samples is None else (int(samples[0]), int(samples[1]))
        if not 0 <= begin < end <= int(spp):
            raise ValueError(f"samples {(begin, end)} must be a non-empty subrange of [0, {int(spp)})")
        workspace = self._workspace(workspace, int(N.lib().zdr_texel_lighting_backward_workspace_bytes(self._handle, H, W)))
        p = N.TexelLightingParams()
        p.struct_size = C.sizeof(N.TexelLightingParams)
        p.tex_h, p.tex_w, p.spp, p.seed, p.sampler = H, W, int(spp), int(seed) & 0xFFFFFFFF, N.SAMPLERS[sampler]
        p.sample_begin, p.sample_end = begin, end
        p.max_distance = 1e30                              # (not looked at)
        N.check(N.lib().zdr_scene_texel_lighting_backward(self._handle, C.byref(p), texel_data.data_ptr(), d_out.data_ptr(),
                                                          None if d_emission is None else d_emission.data_ptr(),
                                                          None if d_env is None else d_env.data_ptr(), workspace.data_ptr(), self._stream()))
        return d_emission, d_env

    class TexelLightingOperator(torch.autograd.Function):
        """texel_lighting() with ``emissions=`` and / or ``envmap=``, modelled on RenderOperator: detached copies become the scene's
        values in the forward, and the backward applies that snapshot again before the native call."""
        @staticmethod
        def forward(ctx, emissions, env, self, texel_data, spp, seed, samples, max_distance):
            if env is not None:
                env = env.detach().clone()
                self.set_envmap_texture(env)
            if emissions is not None:
                self.set_emission_values(emissions.detach().clone())
            ctx.env = env
            ctx.with_emissions = emissions is not None
            ctx.scene = weakref.ref(self)
            ctx.texel_data = texel_data.detach()
            ctx.args = (spp, seed, samples, self.sampler)
            ctx.emissions = self.emissions
            return self.texel_lighting_forward(texel_data, spp=spp, seed=seed, samples=samples, max_distance=max_distance)

        @staticmethod
        def backward(ctx, grad_output):
            scene = ctx.scene()
            if scene.emissions is not ctx.emissions:       # the light list, then its values: the forward's snapshot
                scene.update_lights(ctx.emissions)
            spp, seed, samples, sampler = ctx.args
            d_emission = d_env = None
            if ctx.with_emissions:
                scene._apply_emission_values(ctx.emissions.values)
                d_emission = torch.zeros_like(ctx.emissions.values)
            if ctx.env is not None:
                scene.set_envmap_texture(ctx.env)
                d_env = torch.zeros_like(ctx.env)
            g = grad_output.to(device=scene.device, dtype=torch.float32).contiguous()
            scene.texel_lighting_backward(ctx.texel_data, g, spp=spp, seed=seed, samples=samples, sampler=sampler, d_emission=d_emission, d_env=d_env)
            return d_emission, d_env, None, None, None, None, None, None

    def texel_lighting(self, material, index=0, *, spp=16, seed=0, samples=None, max_distance=None, texels=None, emissions=None, envmap=None) -> TexelLighting:
        """Whether any light reaches each texel of ``material[index]``: a ``TexelLighting`` whose ``data`` is the (H, W, 4) tensor of
        include/zdr.h, zdr_scene_texel_lighting, at that material's size — ``irradiance`` and ``openness``.  ``material`` and ``index``
        are taken as ``texel_aovs`` takes them; ``texels``: a ``TexelAovs`` already computed for them (without it one is computed
        here).  The lights are the scene's current ones (``update_lights``, ``set_emission_values``), the environment map included.

        ``emissions``: a float32 (ninst, 3) tensor on the GPU, ``envmap``: a float32 (H, 2H, 3|4) or (H, H, 3|4) tensor on the GPU, as
        ``render`` takes them — here both may be given in one call.  They become the scene's values, and ``irradiance`` is then
        differentiable in them (include/zdr.h, zdr_scene_texel_lighting_backward): the light list, the sampling tables and visibility
        are held fixed, so for one seed the gradient is exact; its sums use float atomics and may differ in the last bits from run to
        run.  ``openness`` has no gradient.  Without either keyword the call builds no autograd node and returns the bits of
        ``texel_lighting_forward``."""
        if emissions is not None:
            check_emissions(emissions, self.inst_count, self.device)
        env = None if envmap is None else self._prepare_envmap(envmap)
        if texels is None:
            texels = self.texel_aovs(material, index)
        if emissions is None and env is None:
            return TexelLighting(self.texel_lighting_forward(texels.data, spp=spp, seed=seed, samples=samples, max_distance=max_distance))
        return TexelLighting(Scene.TexelLightingOperator.apply(emissions, env, self, texels.data, spp, seed, samples, max_distance))

    # ------------------------------------------------------------------- bounced light
    def _bounce_call(self, texel_data, materials, spp, bounces, seed, samples, sampler, dims, slots):
        """(texel_data, packed materials, dims array, params) of a bounced-light call, checked"""
        if (not isinstance(texel_data, torch.Tensor) or texel_data.ndim != 3 or texel_data.shape[2] != N.AOV_CHANNELS or texel_data.dtype != torch.float32
                or texel_data.device != self.device):
            raise ValueError(f"texel_data must be a float32 (H, W, {N.AOV_CHANNELS}) tensor on {self.device}")
        texel_data = texel_data.detach().contiguous()
        if not 1 <= int(bounces) <= 8:
            raise ValueError(f"bounces is {bounces}, must lie in [1, 8]")
        begin, end = (0, int(spp)) if samples is None else (int(samples[0]), int(samples[1]))
        if not 0 <= begin < end <= int(spp):
            raise ValueError(f"samples {(begin, end)} must be a non-empty subrange of [0, {int(spp)})")
        sampler = self.sampler if sampler is None else sampler
        if sampler not in N.SAMPLERS:
            raise ValueError(f"unknown sampler {sampler!r}")
        if sampler == "pmj02bn":
            self._ensure_pmj_tables()
        packed, d, _ = self._aov_call(materials, dims, slots)
        p = N.TexelBounceParams()
        p.struct_size = C.sizeof(N.TexelBounceParams)
        p.tex_h, p.tex_w, p.spp, p.seed, p.sampler = int(texel_data.shape[0]), int(texel_data.shape[1]), int(spp), int(seed) & 0xFFFFFFFF, N.SAMPLERS[sampler]
        p.sample_begin, p.sample_end, p.bounces = begin, end, int(bounces)
        return texel_data, packed, d, p

    def texel_bounce_forward(self, texel_data, materials, *, spp, bounces=1, seed=0, samples=None, sampler=None, dims=None, slots=None, out=None,
                             workspace=None):
        """The (H, W, 4) buffer of include/zdr.h, zdr_scene_texel_bounce — the irradiance that arrives after 1 .. ``bounces`` Lambertian
        bounces (floats 0..2) and ``surface`` (float 3) — for the surface points of ``texel_data``, an (H, W, 16) tensor in the layout of
        ``texel_aovs_forward``.  ``materials``, ``dims``, ``slots``: as ``render_aovs_forward`` takes them; every material is read, at
        the bounce vertices.  ``samples`` = (begin, end): a subrange of [0, spp) (the outputs of disjoint ranges add up).  ``sampler``:
        "cmj" or "pmj02bn" (default: the scene's).  ``out`` and ``workspace`` (any tensor of at least
        ``zdr_texel_bounce_workspace_bytes`` bytes) are allocated when not given.  This low-level call attaches no gradient
        (``texel_bounce_backward`` is its adjoint, ``texel_bounce`` the differentiable call).  Only enqueues, on torch's current stream."""
        texel_data, packed, d, p = self._bounce_call(texel_data, materials, spp, bounces, seed, samples, sampler, dims, slots)
        workspace = self._workspace(workspace, int(N.lib().zdr_texel_bounce_workspace_bytes(p.tex_h, p.tex_w)))
        out = self._out_tensor(out, (p.tex_h, p.tex_w, 4), False)
        N.check(N.lib().zdr_scene_texel_bounce(self._handle, C.byref(p), texel_data.data_ptr(), packed.data_ptr(), d.ctypes.data, d.shape[0],
                                               out.data_ptr(), workspace.data_ptr(), self._stream()))
        return out

    def texel_bounce_dump(self, texel_data, materials, queries, *, spp, bounces=1, seed=0, samples=None, sampler=None, dims=None, slots=None):
        """zdr_texel_bounce_dump: the walks of ``queries`` (n, 3) int {x, y, s} vertex by vertex, (n, 4 + 12 ``bounces``) float32 in the
        layout of include/zdr.h.  The other arguments are ``texel_bounce_forward``'s.  A test hook."""
        texel_data, packed, d, p = self._bounce_call(texel_data, materials, spp, bounces, seed, samples, sampler, dims, slots)
        q = self._queries(queries)
        out = torch.zeros((q.shape[0], 4 + 12 * p.bounces), dtype=torch.float32, device=self.device)
        N.check(N.lib().zdr_texel_bounce_dump(self._handle, C.byref(p), texel_data.data_ptr(), packed.data_ptr(), d.ctypes.data, d.shape[0],
                                              q.data_ptr(), q.shape[0], out.data_ptr(), self._stream()))
        return out

    def texel_bounce_backward(self, texel_data, d_out, materials, *, spp, bounces=1, seed=0, samples=None, sampler=None, dims=None, slots=None,
                              d_materials=None, d_emission=None, workspace=None):
        """The adjoint of ``texel_bounce_forward``'s irradiance (include/zdr.h, zdr_scene_texel_bounce_backward): with the cotangent
        ``d_out`` (H, W, 4) — float 3, that of ``surface``, is ignored, and so is every texel that is not shaded — ADDS the gradient of
        the material texels' rgb into ``d_materials`` (a list shaped like ``materials``, or the packed buffer; roughness is never
        written) and that of the lights' emissions into ``d_emission``, a float32 (ninst, 3) tensor; one of the two at least.  The
        other arguments are the forward's (the same seed), and the scene must hold the forward's emissions and map.  The walks, the
        light list, the sampling tables, visibility and the acceptance bits are held fixed: for one seed the gradient is the exact
        transpose, also where an albedo is 0.  Not bit-stable from run to run (float atomics).  ``workspace``: any tensor of at least
        ``zdr_texel_bounce_backward_workspace_bytes`` bytes, allocated when not given; it needs no initialisation.  Only enqueues, on
        torch's current stream.  Returns (d_materials, d_emission)."""
        texel_data, packed, d, p = self._bounce_call(texel_data, materials, spp, bounces, seed, samples, sampler, dims, slots)
        H, W = p.tex_h, p.tex_w
        if not isinstance(d_out, torch.Tensor) or tuple(d_out.shape) != (H, W, 4) or d_out.dtype != torch.float32 or d_out.device != self.device:
            raise ValueError(f"d_out must be a float32 ({H}, {W}, 4) tensor on {self.device}")
        d_out = d_out.detach().contiguous()
        if d_materials is None and d_emission is None:
            raise ValueError("texel_bounce_backward needs d_materials, d_emission or both")
        dpacked = None
        if d_materials is not None:
            if isinstance(d_materials, (list, tuple)):
                mats = materials if isinstance(materials, (list, tuple)) else [materials]
                if len(d_materials) != len(mats) or (dims is None and any(tuple(g.shape) != tuple(m.shape) for g, m in zip(d_materials, mats))):
                    raise ValueError("d_materials must be a list shaped like the materials")
            dpacked = self._pack_grads(d_materials, packed)
        if d_emission is not None:
            self._check_d_emission(d_emission, None)
        workspace = self._workspace(workspace, int(N.lib().zdr_texel_bounce_backward_workspace_bytes(self._handle, H, W, d.ctypes.data, d.shape[0])))
        N.check(N.lib().zdr_scene_texel_bounce_backward(self._handle, C.byref(p), texel_data.data_ptr(), d_out.data_ptr(), packed.data_ptr(), d.ctypes.data,
                                                        d.shape[0], None if dpacked is None else dpacked.data_ptr(),
                                                        None if d_emission is None else d_emission.data_ptr(), workspace.data_ptr(), self._stream()))
        if dpacked is not None:
            self._unpack_grads(dpacked, d_materials)
        return d_materials, d_emission

    def texel_bounce_backward_env(self, texel_data, d_out, materials, *, spp, bounces=1, seed=0, samples=None, sampler=None, dims=None, slots=None,
                                  d_env, workspace=None):
        """The adjoint of ``texel_bounce_forward``'s irradiance in the environment map (include/zdr.h,
        zdr_scene_texel_bounce_backward_env): with the cotangent ``d_out`` (H, W, 4) — float 3 and every texel that is not shaded are
        ignored — ADDS the gradient of the map's rgb into ``d_env``, a prepared float32 tensor of the map's size (alpha is never
        touched, and texels that no bounce vertex samples keep their bits).  The other arguments are the forward's (the same seed),
        and the scene must hold the forward's emissions and map.  The bake is linear in the map: with the walks, the sampling tables,
        visibility and the acceptance bits held fixed this is the exact transpose.  A replay of the walk of its own, beside
        ``texel_bounce_backward``'s.  Not bit-stable from run to run (float atomics).  ``workspace``: any tensor of at least
        ``zdr_texel_bounce_backward_env_workspace_bytes`` bytes, allocated when not given; it needs no initialisation.  Only enqueues,
        on torch's current stream.  Returns ``d_env``."""
        texel_data, packed, d, p = self._bounce_call(texel_data, materials, spp, bounces, seed, samples, sampler, dims, slots)
        H, W = p.tex_h, p.tex_w
        if not isinstance(d_out, torch.Tensor) or tuple(d_out.shape) != (H, W, 4) or d_out.dtype != torch.float32 or d_out.device != self.device:
            raise ValueError(f"d_out must be a float32 ({H}, {W}, 4) tensor on {self.device}")
        d_out = d_out.detach().contiguous()
        if not isinstance(d_env, torch.Tensor):
            raise ValueError("texel_bounce_backward_env needs d_env, a prepared float32 tensor of the map's size")
        self._check_d_env(d_env)
        workspace = self._workspace(workspace, int(N.lib().zdr_texel_bounce_backward_env_workspace_bytes(H, W)))
        N.check(N.lib().zdr_scene_texel_bounce_backward_env(self._handle, C.byref(p), texel_data.data_ptr(), d_out.data_ptr(), packed.data_ptr(),
                                                            d.ctypes.data, d.shape[0], d_env.data_ptr(), workspace.data_ptr(), self._stream()))
        return d_env

    class TexelBounceOperator(torch.autograd.Function):
        """texel_bounce() of materials that require grad and / or with ``emissions=`` and / or ``envmap=``, modelled on
        TexelLightingOperator: detached copies of the emissions and of the prepared map become the scene's values in the forward, and
        the backward applies the forward's light list, values and map again before the native calls.  The forward is
        texel_bounce_forward, unchanged."""
        @staticmethod
        def forward(ctx, emissions, self, texel_data, spp, bounces, seed, samples, slots, env, *mats):
            if env is not None:
                env = env.detach().clone()
                self.set_envmap_texture(env)
            if emissions is not None:
                self.set_emission_values(emissions.detach().clone())
            ctx.env = env
            ctx.with_emissions = emissions is not None
            ctx.scene = weakref.ref(self)
            ctx.texel_data = texel_data.detach()
            ctx.args = (spp, bounces, seed, samples, self.sampler, slots)
            ctx.emissions = self.emissions
            ctx.save_for_backward(*mats)
            return self.texel_bounce_forward(texel_data, [m.detach() for m in mats], spp=spp, bounces=bounces, seed=seed, samples=samples, slots=slots)

        @staticmethod
        def backward(ctx, grad_output):
            scene = ctx.scene()
            if scene.emissions is not ctx.emissions:       # the light list, then its values: the forward's snapshot
                scene.update_lights(ctx.emissions)
            spp, bounces, seed, samples, sampler, slots = ctx.args
            mats = [m.detach() for m in ctx.saved_tensors]
            d_emission = d_env = None
            if ctx.with_emissions:
                scene._apply_emission_values(ctx.emissions.values)
                d_emission = torch.zeros_like(ctx.emissions.values)
            if ctx.env is not None:
                scene.set_envmap_texture(ctx.env)
            d_mats = [torch.zeros_like(m) for m in mats] if any(ctx.needs_input_grad[9:]) else None
            g = grad_output.to(device=scene.device, dtype=torch.float32).contiguous()
            if d_mats is not None or d_emission is not None:
                scene.texel_bounce_backward(ctx.texel_data, g, mats, spp=spp, bounces=bounces, seed=seed, samples=samples, sampler=sampler, slots=slots,
                                            d_materials=d_mats, d_emission=d_emission)
            if ctx.env is not None and ctx.needs_input_grad[8]:
                d_env = scene.texel_bounce_backward_env(ctx.texel_data, g, mats, spp=spp, bounces=bounces, seed=seed, samples=samples, sampler=sampler,
                                                        slots=slots, d_env=torch.zeros_like(ctx.env))
            return (d_emission, None, None, None, None, None, None, None, d_env) + (tuple(d_mats) if d_mats is not None else (None,) * len(mats))

    def texel_bounce(self, material, index=0, *, spp=16, bounces=1, seed=0, samples=None, texels=None, emissions=None, envmap=None) -> TexelBounce:
        """The light that reaches each texel of ``material[index]`` after at least one bounce: a ``TexelBounce`` whose ``data`` is the
        (H, W, 4) tensor of include/zdr.h, zdr_scene_texel_bounce, at that material's size — ``irradiance``, the irradiance arriving
        after 1 .. ``bounces`` Lambertian bounces, and ``surface``, the share of the hemisphere that can bounce light at all.
        ``material`` is a tensor or a list exactly as ``render_aovs`` takes it and ``index`` picks the texture that is baked; ALL
        materials are read, at the bounce vertices.  ``texels``: a ``TexelAovs`` already computed for them.  The lights are the
        scene's current ones, the environment map included.  ``albedo / pi * (texel_lighting(...).irradiance + irradiance)`` is the
        Lambertian radiosity of a texel.  Roughness is ignored, and ``bounces`` truncates the walk.

        ``irradiance`` is differentiable in the rgb of every material tensor that requires grad (each receives a gradient of its own
        shape), in ``emissions``, a float32 (ninst, 3) tensor on the GPU that becomes the scene's values as in ``texel_lighting``
        (include/zdr.h, zdr_scene_texel_bounce_backward), and in ``envmap``, a float32 (H, 2H, 3|4) or (H, H, 3|4) tensor on the GPU
        that becomes the scene's map as in ``texel_lighting`` (zdr_scene_texel_bounce_backward_env; its gradient comes back in the
        caller's shape, from a second replay of the walk — ``texel_bounce_backward_env``): the walks, the light list, the sampling
        tables and visibility are held fixed, so for one seed the gradient is exact; its sums use float atomics and may differ in the
        last bits from run to run.  ``surface`` has no gradient, nor have the roughness and the geometry.  With plain tensors and
        without ``emissions`` and ``envmap`` the call builds no autograd node and returns the bits of ``texel_bounce_forward``."""
        if emissions is not None:
            check_emissions(emissions, self.inst_count, self.device)
        env = None if envmap is None else self._prepare_envmap(envmap)
        mats, slots, dims, _ = self._resolve_materials(material, True, pack=False)
        if not 0 <= int(index) < len(dims):
            raise ValueError(f"index {index}: {len(dims)} materials were given")
        if texels is None:
            texels = self.texel_aovs(material, index)
        if emissions is None and env is None and not (torch.is_grad_enabled() and any(m.requires_grad for m in mats)):
            return TexelBounce(self.texel_bounce_forward(texels.data, mats, spp=spp, bounces=bounces, seed=seed, samples=samples, slots=slots))
        return TexelBounce(Scene.TexelBounceOperator.apply(emissions, self, texels.data, spp, bounces, seed, samples, slots, env, *mats))

    # ------------------------------------------------------------- texture-space views
    def texel_view_forward(self, texel_data, res, *, camera=None, out=None, workspace=None):
        """The (H, W, 8) view buffer of include/zdr.h, zdr_scene_texel_view — visible, cosine, pixel x / y, depth, distance, scale, 0 —
        of ``camera`` (default: ``scene.camera``) with an image of ``res`` = (width, height), for the surface points of ``texel_data``,
        an (H, W, 16) tensor in the layout of ``texel_aovs_forward`` of which the normal, the texel size, the position and ``reach``
        are read.  ``out`` and ``workspace`` (any tensor of at least ``zdr_texel_view_workspace_bytes`` bytes) are allocated when not
        given.  ``camera`` may be a camera tensor (10 float32 values on the CPU, ``Camera.to_tensor``): it is read on the host, without
        a synchronisation, and gives the bits of the equivalent ``Camera``; this low-level call attaches no gradient (``texel_view``
        does).  Only enqueues, on torch's current stream."""
        if texel_data.ndim != 3 or texel_data.shape[2] != N.AOV_CHANNELS or texel_data.dtype != torch.float32 or texel_data.device != self.device:
            raise ValueError(f"texel_data must be a float32 (H, W, {N.AOV_CHANNELS}) tensor on {self.device}")
        width, height = int(res[0]), int(res[1])
        if width < 1 or height < 1:
            raise ValueError(f"res must be a positive (width, height), not {res}")
        texel_data = texel_data.detach().contiguous()
        H, W = int(texel_data.shape[0]), int(texel_data.shape[1])
        workspace = self._workspace(workspace, int(N.lib().zdr_texel_view_workspace_bytes(H, W)))
        out = self._out_tensor(out, (H, W, 8), False)
        p = N.TexelViewParams()
        p.struct_size = C.sizeof(N.TexelViewParams)
        p.tex_h, p.tex_w, p.width, p.height = H, W, width, height
        p.camera = _camera_pod(_camera_arg(camera, self.camera)[0])
        N.check(N.lib().zdr_scene_texel_view(self._handle, C.byref(p), texel_data.data_ptr(), out.data_ptr(), workspace.data_ptr(), self._stream()))
        return out

    def texel_view_backward(self, texel_data, d_view, res, *, camera=None, out=None, workspace=None):
        """zdr_texel_view_backward: the adjoint of ``texel_view_forward`` in the camera, a (10,) device tensor in ``Camera.to_tensor``'s
        order (fov, origin, target, up), overwritten, from ``d_view`` (H, W, 8), the cotangent of the view buffer of ``texel_data``.
        ``visible`` is held fixed (float 0 of ``d_view`` is ignored), the rows of texels that are not shaded are not read.  ``camera``:
        a ``Camera`` or a camera tensor (default: ``scene.camera``).  ``out`` and ``workspace`` (any tensor of at least
        ``zdr_texel_view_backward_workspace_bytes`` bytes, contents irrelevant) are allocated when not given.  A deterministic
        reduction without atomics: the same bits from run to run.  Only enqueues, on torch's current stream."""
        if texel_data.ndim != 3 or texel_data.shape[2] != N.AOV_CHANNELS or texel_data.dtype != torch.float32 or texel_data.device != self.device:
            raise ValueError(f"texel_data must be a float32 (H, W, {N.AOV_CHANNELS}) tensor on {self.device}")
        H, W = int(texel_data.shape[0]), int(texel_data.shape[1])
        if not isinstance(d_view, torch.Tensor) or tuple(d_view.shape) != (H, W, 8) or d_view.dtype != torch.float32 or d_view.device != self.device:
            raise ValueError(f"d_view must be a float32 {(H, W, 8)} tensor on {self.device}")
        width, height = int(res[0]), int(res[1])
        if width < 1 or height < 1:
            raise ValueError(f"res must be a positive (width, height), not {res}")
        texel_data, d_view = texel_data.detach().contiguous(), d_view.detach().contiguous()
        workspace = self._workspace(workspace, int(N.lib().zdr_texel_view_backward_workspace_bytes(H, W)))
        out = self._out_tensor(out, (10,), False)
        p = N.TexelViewParams()
        p.struct_size = C.sizeof(N.TexelViewParams)
        p.tex_h, p.tex_w, p.width, p.height = H, W, width, height
        p.camera = _camera_pod(_camera_arg(camera, self.camera)[0])
        N.check(N.lib().zdr_texel_view_backward(C.byref(p), texel_data.data_ptr(), d_view.data_ptr(), out.data_ptr(), workspace.data_ptr(), self._stream()))
        return out

    def texel_view(self, material, index=0, *, res, camera=None, texels=None, footprint=False) -> TexelView:
        """What ``camera`` (default: ``scene.camera``) sees of each texel of ``material[index]`` in an image of ``res`` = (width,
        height): a ``TexelView``.  ``material`` and ``index`` are taken as ``texel_aovs`` takes them; ``texels``: a ``TexelAovs``
        already computed for them (without it one is computed here).  ``footprint=True`` (the same as "square") also computes the footprint buffer
        (``texel_footprint_forward``) and attaches it as ``view.footprint_data``, which ``gather(..., filter="aniso")`` needs: each
        texel as a square patch of side ``texel_size``.  ``footprint="uv"``: each texel as the parallelogram of its UV tangents, which
        follows a non-square texture or a stretched chart (README, "UV tangents"); it takes ``texels.tangents``, computes texels with
        tangents itself when ``texels`` is not given, and raises ``ValueError`` when ``texels`` was made without them.  No
        gradient, unless ``camera`` is a camera tensor that requires grad (10 float32 values on the CPU, ``Camera.to_tensor``; a device
        tensor raises ``ValueError``): then ``view.data`` carries gradient to it — through ``view.gather`` ("bilinear", "mip") and
        ``view.weight()`` — with ``visible`` held fixed, and each backward copies 40 bytes to the host: one synchronisation (README,
        "Camera gradients").  The forward bits are those of the equivalent ``Camera``."""
        if footprint and footprint not in (True, "square", "uv"):
            raise ValueError(f'footprint must be False, True, "square" or "uv", not {footprint!r}')
        patch = None if not footprint else "uv" if footprint == "uv" else "square"
        if texels is None:
            texels = self.texel_aovs(material, index, tangents=patch == "uv")
        elif patch == "uv" and getattr(texels, "tangents", None) is None:
            raise ValueError('footprint="uv" needs texels that carry UV tangents: scene.texel_aovs(..., tangents=True)')
        cam, cam_tensor = _camera_arg(camera, self.camera)
        if cam_tensor is not None and cam_tensor.requires_grad:
            data = TexelViewOperator.apply(cam_tensor, texels.data.detach(), self, (int(res[0]), int(res[1])))
        else:
            data = self.texel_view_forward(texels.data, res, camera=cam)
        if patch is None:
            return TexelView(data, res)
        from .project import texel_footprint_forward
        if patch == "uv":
            return TexelView(data, res, texel_footprint_forward(texels.data, res, cam, tangents=texels.tangents.data), "uv")
        return TexelView(data, res, texel_footprint_forward(texels.data, res, cam), "square")

    def texel_project(self, views, material, index=0, *, cosine_power=1.0, fill=False, texels=None, filter="bilinear", footprint=1.0, max_aniso=8, plan=None,
                      footprint_patch="square") -> TexelProjection:
        """Photographs into texture space ("bake from photographs"): ``views`` is a list of (camera, image) pairs, each image (h, w, 4)
        of the size the camera took it at (sizes may differ from view to view).  Every view is gathered through its ``texel_view`` and
        weighted with ``view.weight(cosine_power)``; the result has ``color`` = sum w_i c_i / sum w_i (0 where the sum is 0),
        ``weight`` = sum w_i and ``count``, the number of views that see each texel, accumulated in list order.  Differentiable in
        the images.  ``fill=True``: ``color`` is push-pull-filled from the texels some view sees (zdr_amd/pushpull.py), which stay
        bit for bit.  ``material``, ``index``, ``texels``: as ``texel_view`` takes them.  ``filter``, ``footprint``: how each view is
        gathered, as ``texel_gather`` takes them; "mip" prefilters the photographs, so that a texel that covers many pixels reads all
        of them (README, "Prefiltered gather"); "aniso" computes each view's footprint buffer itself and gathers with up to
        ``max_aniso`` probes along each texel's long axis (README, "Anisotropic gather"); ``footprint_patch``, "square" or "uv", is what
        those buffers take a texel to be, as ``texel_view(..., footprint=)`` takes it (read by "aniso" only).  ``plan=True``: every view's gradient goes
        through a gather plan of its own (README, "Gather plan").  The views are made in this call, so the plans are too, EVERY call:
        one build and one synchronisation per view, also where no gradient is asked for.  That buys the bit-stable gradient, not
        speed; a loop over fixed cameras keeps its ``TexelView`` objects and calls ``view.gather(image, plan=True)`` instead, which
        builds each plan once.  A camera may be a camera tensor as ``texel_view`` takes it; one that requires grad receives gradient
        (visibility held fixed; "bilinear" and "mip" only, and not with ``plan``)."""
        from .pushpull import push_pull
        if plan not in (None, True):
            raise ValueError("texel_project makes its views itself: plan must be None or True")
        if len(views) == 0:
            raise ValueError("texel_project needs at least one (camera, image) pair")
        if footprint_patch not in ("square", "uv"):
            raise ValueError(f'footprint_patch must be "square" or "uv", not {footprint_patch!r}')
        if texels is None:
            texels = self.texel_aovs(material, index, tangents=filter == "aniso" and footprint_patch == "uv")
        num = weight = count = None
        for camera, image in views:
            if image.dim() != 3 or image.shape[2] != 4:
                raise ValueError(f"every image must be (height, width, 4), not {tuple(image.shape)}")
            view = self.texel_view(material, index, res=(int(image.shape[1]), int(image.shape[0])), camera=camera, texels=texels,
                                   footprint=footprint_patch if filter == "aniso" else False)
            w = view.weight(cosine_power)
            term = w[..., None] * view.gather(image, filter=filter, footprint=footprint, max_aniso=max_aniso, plan=plan)
            num = term if num is None else num + term
            weight = w if weight is None else weight + w
            count = view.visible.clone() if count is None else count + view.visible
        seen = weight > 0
        color = torch.where(seen[..., None], num / torch.where(seen, weight, torch.ones_like(weight))[..., None], torch.zeros_like(num))
        if fill:
            color = push_pull(color, seen)
        return TexelProjection(color, weight, count)

    def render_denoised(self, material, *, res, spp, seed=0, **denoise_kwargs):
        """``render`` followed by the feature-guided denoiser: ``denoise(render(material), render_aovs(material), **denoise_kwargs)``
        with the same ``res``, ``spp`` and ``seed`` for both, so that the guides line up with the image (zdr_amd/denoiser.py for the
        keywords).  Differentiable with respect to ``material`` like ``render``, through the filter's adjoint and, with
        ``demodulate``, through the albedo it divides by.  Any integrator: the feature buffers do not depend on it."""
        from .denoiser import denoise
        image = self.render(material, res=res, spp=spp, seed=seed)
        return denoise(image, self.render_aovs(material, res=res, spp=spp, seed=seed), **denoise_kwargs)

    # ------------------------------------------------------------------------- launching
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _params(self, res, spp, seed, tex_hw, rect=None, samples=None, camera=None, integrator=None, tile_shard=None) -> N.RenderParams:
        if self.sampler == "pmj02bn":
            self._ensure_pmj_tables()
        p = N.RenderParams()
        p.struct_size = C.sizeof(N.RenderParams)
        p.integrator, p.sampler = self._integrator if integrator is None else integrator, N.SAMPLERS[self.sampler]
        p.width, p.height = int(res[0]), int(res[1])
        p.spp, p.seed = int(spp), int(seed) & 0xFFFFFFFF            # seeds are uint32 (App. B-15)
        p.use_tent = int(bool(self.use_tent_filter))
        p.x0, p.y0, p.x1, p.y1 = rect if rect is not None else (0, 0, p.width, p.height)
        p.sample_begin, p.sample_end = samples if samples is not None else (0, p.spp)
        p.max_depth, p.rr_depth = int(self.max_depth), int(self.rr_depth)
        p.camera = _camera_pod(camera if camera is not None else self.camera)
        p.tex_h, p.tex_w = int(tex_hw[0]), int(tex_hw[1])
        p.tile_shard_index, p.tile_shard_count = tile_shard if tile_shard is not None else (0, 1)
        p.prb_mode = N.PRB_MODES[self.prb_mode]
        return p

    def _out_tensor(self, out, shape, zero):
        """The tensor a call writes: ``out`` once checked, or a fresh one of ``shape`` (``zero``: zero-filled)."""
        if out is None:
            return (torch.zeros if zero else torch.empty)(shape, dtype=torch.float32, device=self.device)
        if tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 {shape} tensor on {self.device}")
        return out

    def _workspace(self, workspace, need):
        """The workspace of a call that needs ``need`` bytes (what its ``*_workspace_bytes`` returned: 0 = the sizes were refused):
        ``workspace`` once checked, or a fresh one."""
        if need == 0:
            raise N.ZdrError(f"libzdr_hip error: {N.lib().zdr_last_error().decode()}")
        if workspace is None:
            return torch.empty(need, dtype=torch.uint8, device=self.device)
        if workspace.device != self.device or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need:
            raise ValueError(f"workspace must be a contiguous tensor of at least {need} bytes on {self.device}")
        return workspace

    def _image_out(self, out, res):
        """The image a forward call writes — zero-filled even when the call covers every pixel: a dropped work item must never
        surface as uninitialised memory."""
        return self._out_tensor(out, (int(res[1]), int(res[0]), 4), True)

    def _native_backward(self, p, g, material, dims, d_material, d_env, d_emission):
        """The native backward call of render_backward (``dims`` None) and render_backward_materials (``dims``: the int32 array of
        _material_call), with the one further target that is given."""
        lib = N.lib()
        target, d_target = None, None
        if d_emission is not None:
            self._check_d_emission(d_emission, d_env)
            target, d_target = "emission", d_emission
        elif d_env is not None:
            self._check_d_env(d_env)
            target, d_target = "env", d_env
        fn = {(False, None): lib.zdr_render_backward,
              (False, "env"): lib.zdr_render_backward_env,
              (False, "emission"): lib.zdr_render_backward_emission,
              (True, None): lib.zdr_render_backward_materials,
              (True, "env"): lib.zdr_render_backward_materials_env,
              (True, "emission"): lib.zdr_render_backward_materials_emission}[dims is not None, target]
        args = [self._handle, C.byref(p), g.data_ptr(), material.data_ptr()]
        if dims is not None:
            args += [dims.ctypes.data, dims.shape[0]]
        args.append(d_material.data_ptr())
        if d_target is not None:
            args.append(d_target.data_ptr())
        N.check(fn(*args, self._stream()))

    def _check_material(self, material):
        assert material.ndim == 3 and material.shape[2] == 4           # render.py:160,177
        if material.device != self.device or material.dtype != torch.float32:
            raise ValueError(f"material must be a float32 tensor on {self.device}")

    def render_forward(self, material, res, spp, seed, *, rect=None, samples=None, out=None, kernel=None, tile_shard=None):
        """render.py:159-173.  Returns the (H, W, 4) image; with ``rect``/``samples``/``tile_shard`` only that shard
        is written (other pixels of ``out`` keep their value; a fresh image is zero-filled).  ``tile_shard`` =
        (index, count): the 8x8 tiles of the rectangle numbered index, index + count, ... (include/zdr.h)."""
        self._check_material(material)
        material = material.detach().contiguous()
        image = self._image_out(out, res)
        p = self._params(res, spp, seed, material.shape[0:2], rect, samples, integrator=kernel, tile_shard=tile_shard)
        N.check(N.lib().zdr_render_forward(self._handle, C.byref(p), material.data_ptr(), image.data_ptr(), self._stream()))
        return image

    def render_backward(self, grad_output, d_material, material, res, spp, seed, *, rect=None, samples=None, camera=None, tile_shard=None, d_env=None, d_emission=None):
        """render.py:176-199: accumulates into ``d_material``; uses ``seed + 1`` like the reference (:196).  ``d_env``: a prepared
        (H, H, 4) float32 tensor of the map's size that also accumulates the gradient of the environment map (zdr_render_backward_env;
        path and direct — collocated has no environment term and leaves it alone).  ``d_emission``: a float32 (ninst, 3) tensor that also
        accumulates the gradient of the lights' emissions (zdr_render_backward_emission; rows of models that are not lights receive
        nothing, collocated leaves it alone); not together with ``d_env``."""
        self._check_material(material)
        material = material.detach().contiguous()
        g = grad_output.reshape(res[1], res[0], 4).to(device=self.device, dtype=torch.float32).contiguous()
        assert d_material.is_contiguous() and d_material.shape == material.shape
        if d_material.device != self.device or d_material.dtype != torch.float32:
            raise ValueError(f"d_material must be a float32 tensor on {self.device}")
        p = self._params(res, spp, seed + 1, material.shape[0:2], rect, samples, camera, tile_shard=tile_shard)
        self._native_backward(p, g, material, None, d_material, d_env, d_emission)
        return d_material, None, None, None, None

    def render_stats(self, material, res, spp, seed=0, *, rect=None, samples=None, tile_shard=None) -> dict:
        """Path statistics of one forward pass (camera samples, rays, shaded vertices ...), SURVEY §8d."""
        self._check_material(material)
        material = material.detach().contiguous()
        p = self._params(res, spp, seed, material.shape[0:2], rect, samples, tile_shard=tile_shard)
        cnt = (C.c_uint64 * 8)()
        N.check(N.lib().zdr_render_stats(self._handle, C.byref(p), material.data_ptr(), cnt, self._stream()))
        return dict(zip(N.COUNTER_NAMES, list(cnt)))

    class RenderOperator(torch.autograd.Function):     # render.py:201-223
        """render() of one material (``dims`` None), or of the packed texels of several (``dims``, ``slots``; it returns their packed
        gradient, and torch.cat's own backward hands each material its part).  With a prepared environment map ``env`` also
        differentiable w.r.t. the map, with an (ninst, 3) tensor ``emissions`` w.r.t. the lights' emissions (one of the two at most)."""
        @staticmethod
        def forward(ctx, material, self, res, spp, seed, env, emissions, dims, slots, update_sampling=False):
            if env is not None:                            # the map this forward renders with: uploaded now, saved for the backward
                env = env.detach().clone()
                self.set_envmap_texture(env)
                if update_sampling:                        # tables of THIS map, built on the device; the backward holds them fixed
                    self.update_envmap_sampling(None, compensate_mis=self._env_compensate_mis, on_device=True)
            if emissions is not None:                      # likewise the emissions: a detached copy becomes the scene's values
                self.set_emission_values(emissions.detach().clone())
            ctx.save_for_backward(material)
            ctx.env = env                                  # (a detached copy: kept as it is, not as a saved input)
            ctx.with_emissions = emissions is not None
            ctx.scene = weakref.ref(self)
            ctx.args = (res, spp, seed, dims, slots)
            ctx.camera = self.camera.copy()
            ctx.emissions = self.emissions
            if dims is None:
                return self.render_forward(material.detach(), res, spp, seed)
            return self.render_forward_materials(material, res, spp, seed, dims=dims, slots=slots)

        @staticmethod
        def backward(ctx, grad_output):
            scene = ctx.scene()
            # scene.camera / lights / environment map may have changed between forward and backward: replay the
            # snapshot (camera restored afterwards, lights and map left at the snapshot — render.py:216-222)
            if scene.emissions is not ctx.emissions:
                scene.update_lights(ctx.emissions)
            material, = ctx.saved_tensors
            mat_grad = torch.zeros(material.size(), dtype=material.dtype, device=material.device)
            res, spp, seed, dims, slots = ctx.args
            d_env = d_emission = None
            if ctx.with_emissions:                         # ctx.emissions holds the forward's copy: applied again, whatever happened in between
                scene._apply_emission_values(ctx.emissions.values)
                d_emission = torch.zeros_like(ctx.emissions.values)
            elif ctx.env is not None:
                scene.set_envmap_texture(ctx.env)          # the material gradient depends on the map's values too
                d_env = torch.zeros_like(ctx.env)
            if dims is None:
                scene.render_backward(grad_output, mat_grad, material.detach(), res, spp, seed, camera=ctx.camera, d_env=d_env, d_emission=d_emission)
            else:                                          # slots = the forward's table: uploaded again if material_slots changed in between
                scene.render_backward_materials(grad_output, mat_grad, material.detach(), res, spp, seed, dims=dims, camera=ctx.camera, slots=slots,
                                                d_env=d_env, d_emission=d_emission)
            return mat_grad, None, None, None, None, d_env, d_emission, None, None, None

    def render(self, material, *, res, spp, seed=0, envmap=None, emissions=None, update_sampling=False):
        """Renders the scene; differentiable w.r.t. ``material`` ((Ht, Wt, 4) float32 on the GPU).
        res = (width, height); returns (height, width, 4) (render.py:225-241).

        ``material`` may also be a list or tuple of such tensors (sizes may differ): model i is then shaded by material
        ``material_slots[i]``, or — with ``material_slots`` unset — the k-th non-emitting model by the k-th material (the list
        must then hold one material per non-emitting model).  With ``material_slots`` set a single tensor is a one-element list.

        ``envmap``: a float32 tensor on the GPU, (H, 2H, 3|4) or (H, H, 3|4), that the render uses as the environment map and
        differentiates (path and direct; collocated sees no environment).  It is prepared as add_envmap prepares an image (alpha 1
        for RGB, a 1:2 map made square), must then have the size given to add_envmap, and becomes the scene's map: later renders
        without ``envmap=`` use it too.  The importance-sampling tables stay those of add_envmap or of the last
        update_envmap_sampling, and the gradient holds them fixed.  At most 15 materials with ``envmap=``.
        ``update_sampling=True`` rebuilds the tables from this map on the GPU (update_envmap_sampling, on_device, with the
        ``compensate_mis`` the tables were last built with) right after the forward uploads it; the gradient still holds them fixed,
        which is exact for the rendered seed and unbiased overall: the estimator's expectation does not depend on the sampling density.

        ``emissions``: a float32 (ninst, 3) tensor on the GPU whose rows the render uses as the emission of the models that are lights
        now (the light list of ``Scene(...)`` or of the last ``update_lights``) and differentiates (path and direct; collocated reads
        no emission and returns a zero gradient).  Rows of other models are ignored and receive gradient 0: which models emit is not
        differentiable, and ``update_lights`` stays the way to change it.  The values become the scene's emissions, for later renders
        without ``emissions=`` too.  For one seed the render is linear in the emissions and the gradient is exact as long as every
        light keeps at least one positive component (zero or negative components are fine; this is not checked).  Not together
        with ``envmap=``."""
        if emissions is not None:
            check_emissions(emissions, self.inst_count, self.device, envmap)
        if update_sampling and envmap is None:
            raise ValueError("update_sampling=True needs envmap=: it rebuilds the tables of the map this call uploads")
        env = None if envmap is None else self._prepare_envmap(envmap)
        if not isinstance(material, (list, tuple)) and self._material_slots is None:
            return Scene.RenderOperator.apply(material, self, res, spp, seed, env, emissions, None, None, bool(update_sampling))
        nmat = len(material) if isinstance(material, (list, tuple)) else 1
        if env is not None and nmat > N.MAX_MATERIALS - 1:
            raise ValueError(f"{nmat} materials given with envmap=: at most {N.MAX_MATERIALS - 1} (the map takes the last entry of the material table)")
        _, slots, dims, packed = self._resolve_materials(material)
        return Scene.RenderOperator.apply(packed, self, res, spp, seed, env, emissions, dims, slots, bool(update_sampling))

    def render_duvdxy(self, material, *, res, spp, seed=0):
        """Gradient of the texture coordinates w.r.t. screen-space coordinates: a (height, width, 4) tensor
        holding (dudx, dvdx, dudy, dvdy) (render.py:243-257, uvgrad.py).  Not differentiable.  The
        reference drives this kernel with LuisaCompute's own random sampler (uvgrad.py:82, third-party);
        here the scene's sampler provides the pixel jitter."""
        return self.render_forward(material.detach(), res, spp, seed, kernel=N.UVGRAD)

    def check(self):
        """Synchronises and raises ZdrError if a device watchdog ended work early since the last check
        (include/zdr.h, zdr_scene_check).  LuisaCompute raises from luisa.synchronize() (render.py:172,198)."""
        N.check(N.lib().zdr_scene_check(self._handle, self._stream()))

    # ------------------------------------------------------------------- test / debug hooks
    def _rays(self, rays):
        assert rays.ndim == 2 and rays.shape[1] == 8
        return rays.to(device=self.device, dtype=torch.float32).contiguous()

    def trace_closest(self, rays):
        """rays: (n, 8) float32 cuda {o, tmin, d, tmax} -> (inst_prim (n,2) int32, bary_t (n,3) float32)."""
        rays = self._rays(rays)
        n = rays.shape[0]
        ip = torch.empty((n, 2), dtype=torch.int32, device=self.device)
        bt = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        N.check(N.lib().zdr_trace_closest(self._handle, rays.data_ptr(), n, ip.data_ptr(), bt.data_ptr(), self._stream()))
        return ip, bt

    def trace_any(self, rays):
        rays = self._rays(rays)
        occ = torch.empty((rays.shape[0],), dtype=torch.int32, device=self.device)
        N.check(N.lib().zdr_trace_any(self._handle, rays.data_ptr(), rays.shape[0], occ.data_ptr(), self._stream()))
        return occ

    def trace_fused(self, shadow, nxt, need, backward_layout=False):
        """The fused walk of the BVH path kernels (include/zdr.h, zdr_trace_fused): row i of ``shadow`` / ``nxt`` ((n, 8) float32) is the
        shadow / continuation ray of lane i % 64 of wave i // 64, ``need`` (n,) int32 says which of the two it has (bit 0 / bit 1)
        -> (occluded (n,) int32, inst_prim (n, 2) int32, bary_t (n, 3) float32)."""
        shadow, nxt = self._rays(shadow), self._rays(nxt)
        need = need.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        n = shadow.shape[0]
        assert nxt.shape[0] == n and need.shape[0] == n
        occ = torch.empty((n,), dtype=torch.int32, device=self.device)
        ip = torch.empty((n, 2), dtype=torch.int32, device=self.device)
        bt = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        N.check(N.lib().zdr_trace_fused(self._handle, shadow.data_ptr(), nxt.data_ptr(), need.data_ptr(), n, 1 if backward_layout else 0,
                                        occ.data_ptr(), ip.data_ptr(), bt.data_ptr(), self._stream()))
        return occ, ip, bt

    SHADING_MODES = {"eval": 0, "sample": 1, "frame": 2}

    def shading_dump(self, mode, rows):
        """The shading math point by point (include/zdr.h, zdr_shading_dump): ``mode`` "eval" | "sample" | "frame", ``rows`` (n, 16)
        float32 laid out as the header says -> (n, 16) float32.  No geometry is read; the scene only names the device."""
        rows = rows.to(device=self.device, dtype=torch.float32).contiguous()
        assert rows.ndim == 2 and rows.shape[1] == 16, rows.shape
        out = torch.empty_like(rows)
        N.check(N.lib().zdr_shading_dump(self._handle, self.SHADING_MODES[mode], rows.data_ptr(), rows.shape[0], out.data_ptr(), self._stream()))
        return out

    LIGHT_MODES = {"sample": 0, "pdf": 1, "env": 2, "misc": 3, "interact": 4, "interact_wide": 5}

    def light_dump(self, mode, rows):
        """The light side of a path vertex point by point (include/zdr.h, zdr_light_dump): ``mode`` "sample" | "pdf" | "env" | "misc" |
        "interact" | "interact_wide", ``rows`` (n, 16) float32 laid out as the header says -> (n, 16) float32, computed with this
        scene's light table, environment map and acceleration structure."""
        rows = rows.to(device=self.device, dtype=torch.float32).contiguous()
        assert rows.ndim == 2 and rows.shape[1] == 16, rows.shape
        out = torch.empty_like(rows)
        N.check(N.lib().zdr_light_dump(self._handle, self.LIGHT_MODES[mode], rows.data_ptr(), rows.shape[0], out.data_ptr(), self._stream()))
        return out

    SCATTER_FORMS = {"single": 0, "table": 1, "table_env": 2}

    def _texture_table(self, sizes):
        dims = np.ascontiguousarray(np.array(sizes, np.int32).reshape(-1, 2))
        return dims, int(sum(int(h) * int(w) for h, w in dims))

    def texture_lookup(self, materials, sizes, rows):
        """The bilinear lookups row by row (include/zdr.h, zdr_texture_lookup): ``materials`` the packed texels ((sum h w, 4) float32) of the
        table ``sizes`` [(h, w), ...], ``rows`` (n, 3 or 4) float32 {u, v, bits(material index)} -> (n, 20) float32 {read_bsdf narrow, wide,
        read_bsdf_in narrow, wide, env_lookup[3], 0}."""
        dims, texels = self._texture_table(sizes)
        materials = materials.to(device=self.device, dtype=torch.float32).contiguous()
        assert materials.numel() == 4 * texels, (materials.shape, texels)
        r = torch.zeros((rows.shape[0], 4), dtype=torch.int32, device=self.device)        # (bits, not values: the index is no number)
        r[:, :3] = rows.to(device=self.device, dtype=torch.float32).contiguous().view(torch.int32)[:, :3]
        out = torch.empty((r.shape[0], 20), dtype=torch.float32, device=self.device)
        N.check(N.lib().zdr_texture_lookup(self._handle, materials.data_ptr(), dims.ctypes.data, dims.shape[0], r.data_ptr(), r.shape[0], out.data_ptr(), self._stream()))
        return out

    def texture_scatter(self, form, sizes, rows, rounds, d_materials, d_env=None):
        """The staging-cell scatter and the fold row by row (include/zdr.h, zdr_texture_scatter): ``form`` "single" | "table" | "table_env",
        ``rows`` (n, 7 or 8) float32 {u, v, g[4], bits(material index)}; adds into ``d_materials`` ((sum h w, 4) float32 cuda, in place) and,
        third form, into ``d_env`` ((env_h, env_w, 4)) -> the copies of the staging cells each of the 16 table entries was given."""
        dims, texels = self._texture_table(sizes)
        assert d_materials.is_cuda and d_materials.dtype == torch.float32 and d_materials.is_contiguous() and d_materials.numel() == 4 * texels
        assert d_env is None or (d_env.is_cuda and d_env.dtype == torch.float32 and d_env.is_contiguous())
        r = torch.zeros((rows.shape[0], 8), dtype=torch.int32, device=self.device)        # (bits, not values: the index is no number)
        r[:, :7] = rows.to(device=self.device, dtype=torch.float32).contiguous().view(torch.int32)[:, :7]
        copies = np.zeros(N.MAX_MATERIALS, np.int32)
        N.check(N.lib().zdr_texture_scatter(self._handle, self.SCATTER_FORMS[form], dims.ctypes.data, dims.shape[0], r.data_ptr(), r.shape[0], int(rounds),
                                            d_materials.data_ptr(), None if d_env is None else d_env.data_ptr(), copies.ctypes.data, self._stream()))
        return copies

    def _queries(self, queries):
        """(n, 3) int32 {px, py, sample_index} on the scene's device, contiguous."""
        return queries.reshape(-1, 3).to(device=self.device, dtype=torch.int32).contiguous()

    def sampler_dump(self, queries, spp, seed=0, nvert=3, rr_depth=RR_DEPTH):
        """queries: (n, 3) int32 cuda {px, py, sample_index} -> (n, 2 + 8*nvert) float32 sampler draws."""
        q = self._queries(queries)
        out = torch.empty((q.shape[0], 2 + 8 * nvert), dtype=torch.float32, device=self.device)
        N.check(N.lib().zdr_sampler_dump(self._handle, N.SAMPLERS[self.sampler], int(seed) & 0xFFFFFFFF, int(spp), q.data_ptr(), q.shape[0], nvert, rr_depth, out.data_ptr(), self._stream()))
        return out

    def vertex_sampler_dump(self, queries, spp, seed=0, nvert=3, rr_depth=RR_DEPTH, integrator="path"):
        """As sampler_dump, but drawn the way the path (or the direct) kernels draw (include/zdr.h, zdr_vertex_sampler_dump).
        Returns (draws, batched): batched is True when the packed two-permutations-per-register route ran."""
        q = self._queries(queries)
        out = torch.empty((q.shape[0], 2 + 8 * nvert), dtype=torch.float32, device=self.device)
        b = C.c_int32(-1)
        N.check(N.lib().zdr_vertex_sampler_dump(self._handle, N.INTEGRATORS[integrator], N.SAMPLERS[self.sampler], int(seed) & 0xFFFFFFFF, int(spp), q.data_ptr(), q.shape[0], nvert, rr_depth, out.data_ptr(), C.byref(b), self._stream()))
        return out, bool(b.value)

    def path_dump(self, material, queries, res, spp, seed, *, d_image=None, maxv=16):
        """Per-path traces (include/zdr.h, zdr_path_dump): queries (n, 3) int32 cuda {px, py, sample_index} ->
        (n, 8 + 24 maxv) float32.  ``seed`` is used as it is (pass seed + 1 for the paths of a backward pass)."""
        self._check_material(material)
        material = material.detach().contiguous()
        q = self._queries(queries)
        out = torch.empty((q.shape[0], 8 + 24 * maxv), dtype=torch.float32, device=self.device)
        p = self._params(res, spp, seed, material.shape[0:2])
        g = None if d_image is None else d_image.reshape(res[1], res[0], 4).to(device=self.device, dtype=torch.float32).contiguous()
        N.check(N.lib().zdr_path_dump(self._handle, C.byref(p), material.data_ptr(), None if g is None else g.data_ptr(), q.data_ptr(), q.shape[0], maxv, out.data_ptr(), self._stream()))
        return out
