"""One clip, end to end, as three separable stages over the HIP-backed mirror:

    cond    = Conditions.build(model, videos, ...)       # embedders + first / last frame through the encoder
    latents = sample(model, cond, plan)                  # DDIM (two- or three-way guidance; pinned= holds extra keyframes)
    video   = decode_spliced(model, latents, cond.refs)  # 16-frame decode + 14-frame re-decode, centre frames spliced

`bench.py` times the second and third stage on resident conditioning; `synthesize` chains all three.  Callers that hold
uint8 frames on the device start at `Conditions.from_uint8` / `synthesize_u8`: the script's PIL transform and the image
tower's preprocessing run as HIP kernels there (tc_frames_from_u8, tc_clip_patches).  The caller the
reference ships for this path is `image_guided_synthesis` (scripts/evaluation/inference.py:180-277, with its helper
`get_latent_z_with_hidden_states`, :164-178); `image_guided_synthesis` below keeps that call signature (argument names and
order are the interface of the reference's scripts) and is a thin adapter onto the stages.  The unmodified script's own copy
also runs on the mirror (tests/test_dropin_run_cpu.py), so nothing here is needed for the drop-in: this module is the API
for callers that hold conditioning resident and run many clips (bench.py, dist.py).

Result-preserving restructuring: the reference encodes all T frames and keeps frames 0 and T-1 of the latent and of the
hidden states; only those two frames are encoded here (8x less encoder work at T = 16).
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import List, Optional, Sequence

import torch

from . import ops
from .lvdm.attention import check_frames
from .lvdm.ddim import DDIMSampler
from .lvdm.ddim_multiplecond import DDIMSampler as ThreeWaySampler
from .output import Colour, clip_to_uint8, hold_still, match_colour, write_frames


def encode_endpoints(model, videos):
    """(b, c, t, h, w) pixels -> (z_first, z_last) latents of frames 0 and t-1, each (b, 4, h/8, w/8), and the encoder's
    hidden states of those two frames as (b, C, 2, H, W) tensors: the decoder's reference features."""
    b, c, t, h, w = videos.shape
    ends = torch.stack([videos[:, :, 0], videos[:, :, t - 1]], 1).reshape(2 * b, c, h, w)
    posterior, hidden = model.first_stage_model.encode(ends, return_hidden_states=True)
    z = model.get_first_stage_encoding(posterior).detach().unflatten(0, (b, 2))
    refs = [hdn.unflatten(0, (b, 2)).transpose(1, 2).contiguous() for hdn in hidden]
    return z[:, 0], z[:, 1], refs


@dataclass
class Conditions:
    """Everything the sampler and the decoder consume, resident on the device."""
    positive: dict                       # text + image tokens, concat latents
    negative: Optional[dict]             # the unconditional branch (None when guidance is off)
    image_only: Optional[dict]           # third branch of the three-way guidance (image yes, text "")
    refs: Optional[List[torch.Tensor]]   # decoder reference features
    fs: torch.Tensor
    endpoints: Optional[torch.Tensor] = field(default=None, repr=False)    # (b, 4, t, h, w), frames 0 / t-1 filled
    three_way: bool = False              # sampler family (the reference picks it by flag, not by the branch's presence)
    # (b, 3, 2, H, W): the pixels of the two keyframes at model size, what `match=` matches the decoded clip to (a small copy of
    # frames 0 and t-1 of `videos`; without hold_endpoints both slots hold frame 0)
    ends_px: Optional[torch.Tensor] = field(default=None, repr=False)

    @staticmethod
    def build(model, videos, *, prompts=None, fs=None, guided=True, three_way=False, image_branch=True, hold_endpoints=True,
              embed=None):
        """`hold_endpoints`: frames 0 AND t-1 condition the clip (interpolation / looping); otherwise frame 0 is repeated
        over time (plain image-to-video).  `embed`: the image tower, (b, 3, H, W) pixels -> tokens (default: `model.embedder`)."""
        b, t = videos.shape[0], videos.shape[2]
        prompts = list(prompts) if prompts is not None else [""] * b
        first = videos[:, :, 0]
        embed = model.embedder if embed is None else embed

        def tokens(text_emb, image):
            return torch.cat([text_emb, model.image_proj_model(embed(image))], dim=1)

        text = model.get_learned_conditioning(prompts)
        pos = {"c_crossattn": [tokens(text, first)]}
        neg = img_only = refs = canvas = None
        hybrid = model.model.conditioning_key == "hybrid"
        if hybrid:
            z0, z1, refs = encode_endpoints(model, videos)
            if hold_endpoints:
                canvas = z0.new_zeros((b, z0.shape[1], t, *z0.shape[2:]))
                canvas[:, :, 0], canvas[:, :, t - 1] = z0, z1
            else:
                canvas = z0.unsqueeze(2).expand(-1, -1, t, -1, -1).contiguous()
            pos["c_concat"] = [canvas]
        if guided:
            if model.uncond_type == "empty_seq":
                blank = model.get_learned_conditioning([""] * b)
            elif model.uncond_type == "zero_embed":
                blank = torch.zeros_like(text)
            else:
                raise NotImplementedError(f"uncond_type {model.uncond_type!r}")
            neg = {"c_crossattn": [tokens(blank, torch.zeros_like(first))]}
            if three_way and image_branch:
                img_only = {"c_crossattn": [torch.cat([blank, pos["c_crossattn"][0][:, text.shape[1]:]], dim=1)]}
            if hybrid:                              # the SAME tensor object: apply_model_multi shares the prefix on it
                for branch in (neg, img_only):
                    if branch is not None:
                        branch["c_concat"] = [canvas]
        fs_t = torch.full((b,), int(fs), dtype=torch.long, device=model.device) if not torch.is_tensor(fs) else fs
        ends_px = torch.stack([first, videos[:, :, t - 1] if hold_endpoints else first], dim=2)
        return Conditions(pos, neg, img_only, refs, fs_t, canvas, three_way, ends_px)

    @staticmethod
    def from_uint8(model, first_u8, last_u8, *, size, t, **options):
        """`build` from uint8 frames on the device: `first_u8` / `last_u8` are (b, h, w, 3) uint8 keyframes of any size (what
        `clip_to_uint8` returns, or a decoder's output), `size` the model's (H, W).  They become frames 0 and t-1 of the clip
        tensor by the script's transform (`frames_from_uint8`); the encoder runs as in `build` and the image tower takes its
        patches from tc_clip_patches (`encode_on_device_front`).  `options`: the keyword options of `build` other than `embed`."""
        _check_images("from_uint8: first_u8", first_u8, "b")
        _check_images("from_uint8: last_u8", last_u8, "b")
        return Conditions._from_keyframes("from_uint8", frames_from_uint8, model, first_u8, last_u8, size, t, options)

    @staticmethod
    def from_planes(model, first, last, *, size, t, **options):
        """`from_uint8` for planar 4:2:0 keyframes on the device: `first` / `last` are `Planes` of b images each (a decoder's
        NV12 / P010 surfaces, or `planes_from_packed` of a planar clip).  They become frames 0 and t-1 by `frames_from_planes`;
        the encoder and the image tower run as in `from_uint8`."""
        for name, planes in (("first", first), ("last", last)):
            if not isinstance(planes, Planes):
                raise ValueError(f"from_planes: {name} must be a Planes, got {type(planes).__name__}")
        return Conditions._from_keyframes("from_planes", frames_from_planes, model, first, last, size, t, options)

    @staticmethod
    def _from_keyframes(what, frames, model, first, last, size, t, options):
        """The shared tail of from_uint8 / from_planes: b first and b last keyframes become frames 0 and t-1 of the clip tensor
        by `frames` (frames_from_uint8 or frames_from_planes), then `build` with the image tower on the device front."""
        b = len(first)
        if b != len(last):
            raise ValueError(f"{what}: {b} first frames, {len(last)} last frames")
        videos = frames(first, size, [(i, 0) for i in range(b)], t)
        frames(last, size, [(i, t - 1) for i in range(b)], t, out=videos)
        return Conditions.build(model, videos, embed=model.embedder.encode_on_device_front, **options)


@dataclass(eq=False)
class Planes:
    """n planar 4:2:0 images as a hardware decoder (or `clip_to_uint8(fmt="i420" | "nv12")`) leaves them:
      fmt "i420": y (n, h, w) uint8, chroma = (Cb, Cr), each (n, ch, cw) uint8, one pitch for both;
      fmt "nv12": y (n, h, w) uint8, chroma = (CbCr,), (n, ch, cw, 2) uint8;
      fmt "p010": the nv12 shapes with 2-byte elements (torch.uint16 or torch.int16: the bits are what is read), the sample
                  in the upper ten bits of each little-endian word -- a P016 surface of a 10-bit stream;
    ch = (h + 1) // 2, cw = (w + 1) // 2.  Row-strided views are taken as they are (the pitch is the stride); inside a row the
    stride is one.  `standard` "bt601" | "bt709" and `range` "limited" | "full" pick the integer matrix (tc_yuv_matrix), or
    `matrix` gives its seven integers; `siting` "nearest" | "center" | "left" where the chroma samples sit.
    Wrong dtypes, shapes or strides raise ValueError here, before anything is launched."""
    y: torch.Tensor
    chroma: tuple
    fmt: str
    standard: str = "bt601"
    range: str = "limited"
    siting: str = "center"
    matrix: Optional[Sequence[int]] = None

    def __post_init__(self):
        self.chroma = tuple(self.chroma) if isinstance(self.chroma, (tuple, list)) else (self.chroma,)
        ops.planes_layout(self, "Planes")

    def __len__(self):
        return self.y.shape[0]

    def __getitem__(self, index):
        """images `index` (a slice) as a Planes over the same memory"""
        if not isinstance(index, slice):
            raise TypeError("Planes: index with a slice (planes[i:i + 1] for one image)")
        return Planes(self.y[index], tuple(c[index] for c in self.chroma), self.fmt, self.standard, self.range, self.siting, self.matrix)


def _check_images(what, images, n="n", planes=False):
    """`images` as the pixel front end takes them, or ValueError under the caller's name `what`: (n, h, w, 3) uint8 (`n`: the
    caller's letter for the count), or, with `planes`, a `Planes`."""
    if planes and isinstance(images, Planes):
        return
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise ValueError(f"{what} must be ({n}, h, w, 3) uint8{' or a Planes' if planes else ''}, got "
                         f"{tuple(images.shape) if isinstance(images, torch.Tensor) else type(images).__name__} {getattr(images, 'dtype', '')}")


def _packed_frames(what, buf, h, w, sample_bytes):
    """The checked buffers of `what` (planes_from_packed / planes_from_frames): (h, w, the frames as rows), for a positive even
    size and uint8 (..., h * w * 3 / 2 * sample_bytes) buffers with unit stride, flattened without a copy to (frames, samples) --
    uint8 samples, or for sample_bytes = 2 the 2-byte words of P010."""
    h, w = int(h), int(w)
    if h <= 0 or w <= 0 or h % 2 or w % 2:
        raise ValueError(f"{what}: the packed planar formats have an even size, got {(h, w)}")
    n = h * w * 3 // 2 * sample_bytes
    if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or buf.dim() < 1 or buf.shape[-1] != n or buf.stride(-1) != 1:
        raise ValueError(f"{what}: expected uint8 (..., {n}) {'P010 ' if sample_bytes == 2 else ''}frames with unit stride, got "
                         f"{tuple(buf.shape) if isinstance(buf, torch.Tensor) else type(buf)} {getattr(buf, 'dtype', '')}")
    try:
        rows = buf.view(-1, n)
        return h, w, rows if sample_bytes == 1 else rows.view(torch.uint16)
    except RuntimeError as e:
        raise ValueError(f"{what}: the frames do not flatten{' into 2-byte words' if sample_bytes == 2 else ''} without a copy (strides {buf.stride()}, "
                         f"offset {buf.storage_offset()})") from e


def planes_from_packed(buf, h, w, fmt, **options):
    """Views (no copy) of the (..., h * w * 3 / 2) uint8 buffers `clip_to_uint8(fmt="i420" | "nv12")` returns as a `Planes` of
    all their frames, in order: a planar clip's last frame is `planes_from_packed(clip[:, -1], h, w, fmt)`.  The back end writes
    BT.601 limited range from 2 x 2 means, which the defaults (`options`: standard, range, siting) undo."""
    if fmt not in ("i420", "nv12"):
        raise ValueError(f"planes_from_packed: fmt {fmt!r}: 'i420' or 'nv12'")
    h, w, flat = _packed_frames("planes_from_packed", buf, h, w, 1)
    n, q = h * w, (h // 2) * (w // 2)
    y = flat[:, :n].unflatten(1, (h, w))
    if fmt == "i420":
        chroma = (flat[:, n:n + q].unflatten(1, (h // 2, w // 2)), flat[:, n + q:].unflatten(1, (h // 2, w // 2)))
    else:
        chroma = (flat[:, n:].unflatten(1, (h // 2, w // 2, 2)),)
    return Planes(y, chroma, fmt, **options)


def planes_from_frames(buf, h, w, fmt, colour):
    """`planes_from_packed` for the frames `clip_to_uint8(..., colour=)` / `synthesize_u8(..., out_colour=)` return: views (no
    copy) of the uint8 (..., bytes per frame) buffers as a `Planes` carrying the colour's standard / range / siting, so that a
    clip's last frame is the next clip's keyframe in the same description.  colour.bits == 10: the (..., h * w * 3) bytes of
    P010 frames, viewed as fmt "p010" with 2-byte elements (`fmt` is then "nv12", as it was for the call that wrote them)."""
    if not isinstance(colour, Colour):
        raise ValueError(f"planes_from_frames: colour: expected a Colour, got {type(colour).__name__}")
    options = dict(standard=colour.standard, range=colour.range, siting=colour.siting)
    if colour.bits == 8:
        return planes_from_packed(buf, h, w, fmt, **options)
    if fmt != "nv12":
        raise ValueError(f"planes_from_frames: fmt {fmt!r}: 10-bit frames are 'nv12' in 2-byte words (P010)")
    h, w, words = _packed_frames("planes_from_frames", buf, h, w, 2)
    n = h * w
    return Planes(words[:, :n].unflatten(1, (h, w)), (words[:, n:].unflatten(1, (h // 2, w // 2, 2)),), "p010", **options)


def frames_from_planes(planes, size, slots, t, out=None):
    """`frames_from_uint8` for a `Planes` of n images: chroma upsample and YCbCr -> RGB in integers, then the script's
    transform of that RGB image, bit for bit, on the device (tc_frames_from_yuv)."""
    if not isinstance(planes, Planes):
        raise ValueError(f"frames_from_planes: expected a Planes, got {type(planes).__name__}")
    size, flat, b, t = _clip_slots("frames_from_planes", len(planes), size, slots, t, out)
    return ops.frames_from_yuv(planes, size, flat, b=b, t=t, out=out)


def _clip_slots(what, n, size, slots, t, out):
    """The checked request of `what` (frames_from_uint8 / frames_from_planes) for n images: (size, the slots as batch * t + frame,
    b, t), b from `out` or 1 + the largest batch index."""
    size, slots, t = tuple(int(v) for v in size), [(int(i), int(f)) for i, f in slots], int(t)
    if len(size) != 2 or min(size) <= 0 or t <= 0:
        raise ValueError(f"{what}: size {size}, t {t}")
    if len(slots) != n or any(i < 0 or not 0 <= f < t for i, f in slots):
        raise ValueError(f"{what}: {n} images need as many (batch, frame) slots with frame < {t}, got {slots}")
    b = out.shape[0] if out is not None else 1 + max(i for i, _ in slots)
    if any(i >= b for i, _ in slots):
        raise ValueError(f"{what}: slots {slots} for a batch of {b}")
    return size, [i * t + f for i, f in slots], b, t


def frames_from_uint8(images_u8, size, slots, t, out=None):
    """uint8 (n, h, w, 3) device images -> the (b, 3, t, H, W) fp32 clip tensor the model takes, `size` = (H, W): image i fills
    the (batch, frame) pair slots[i] by the script's transform (inference.py:64-69: Resize(min(size)), CenterCrop(size),
    ToTensor, Normalize(0.5, 0.5) on PIL images), bit for bit, on the device.  b = 1 + the largest batch index; frames no slot
    names are zero.  `out`: a clip tensor to fill in place instead (the frames no slot names keep their contents)."""
    _check_images("frames_from_uint8: images_u8", images_u8)
    size, flat, b, t = _clip_slots("frames_from_uint8", images_u8.shape[0], size, slots, t, out)
    return ops.frames_from_u8(images_u8, size, flat, b=b, t=t, out=out)


@dataclass
class SamplingPlan:
    steps: int = 50
    eta: float = 1.0
    scale: float = 7.5                     # 1.0 = no guidance
    image_scale: Optional[float] = None    # three-way guidance only
    spacing: str = "uniform_trailing"
    rescale: float = 0.7
    extra: dict = field(default_factory=dict)
    # one integer in [0, 2^64) per clip of the batch: every Gaussian draw of clip i then comes from tc_randn_clips keyed by
    # seeds[i] (stream numbering: lvdm/ddim.py), so the clip is the same in any batch, slot or rank and the torch generator
    # is not touched.  Philox noise, not torch's: it does not reproduce a reference run with seed_everything -- None does.
    seeds: Optional[Sequence[int]] = None
    # solver order: 1 = the reference's DDIM update; 2 = the second-order multistep correction from the previous step's
    # pred_x0 (tc_ddim_step_ms; no further UNet call), meant for runs of fewer steps.  Opt-in: verified on an analytic
    # model only, its effect on real frames at reduced step counts is unmeasured.
    order: int = 1


_MASK64 = (1 << 64) - 1


def variant_seed(seed: int, k: int) -> int:
    """The seed of variant `k` of the clip seeded `seed` (`synthesize(..., variants=)`), a pure function so that variant 3
    can be regenerated alone: k = 0 is the seed itself; k > 0 is the splitmix64 finaliser of seed + k * 0x9E3779B97F4A7C15
    mod 2^64:  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31  (all mod 2^64)."""
    seed, k = int(seed), int(k)
    if not 0 <= seed <= _MASK64 or k < 0:
        raise ValueError(f"variant_seed: seed {seed} outside [0, 2^64) or variant {k} < 0")
    if k == 0:
        return seed
    z = (seed + k * 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def pin_frames(model, frames, t):
    """Extra keyframes for `sample(..., pinned=...)`: `frames` maps a frame index to (b, 3, H, W) pixels in [-1, 1].  They
    go through the first-stage encoder (one call) and come back as the sampler's pair: x0 (b, 4, t, h, w), zero away from
    those frames, and mask (b, 1, t, 1, 1), one on them."""
    index = sorted(int(i) for i in frames)
    if not index or index[0] < 0 or index[-1] >= t:
        raise IndexError(f"keyframe indices {index} for a clip of {t} frames")
    z = model.encode_first_stage(torch.stack([frames[i] for i in index], dim=2)).to(torch.float32)     # (b, 4, k, h, w)
    x0 = z.new_zeros((z.shape[0], z.shape[1], t, *z.shape[3:]))
    mask = z.new_zeros((z.shape[0], 1, t, 1, 1))
    x0[:, :, index] = z
    mask[:, :, index] = 1.0
    return x0, mask


@dataclass(frozen=True)
class StillRegions:
    """What the `still=` keyword of the synthesis calls holds between two keyframes (the rule: include/tooncrafter_hip.h,
    tc_still_map): a pixel has moved if a channel of the two keyframes differs by more than `tau` 8-bit code values, an 8 x 8
    cell (one latent position) if any of its pixels has; the moving area is grown by `grow` cells and the pixel weight rises
    from 0 to 1 over the next `feather` cells.  `pin`: the still cells' latents are held during sampling (`still_pins`);
    `composite`: the still pixels of the decoded clip are the keyframes' own, feathered (`output.hold_still`).
    The defaults are starting values.  Nobody has measured them on real footage: no claim is made about what they do to real
    ToonCrafter frames.  Nothing is motion compensated: a panned background has moved."""
    tau: int = 8
    grow: int = 1
    feather: int = 2
    pin: bool = True
    composite: bool = True

    def __post_init__(self):
        ops.HipOps.still_rule(self.tau, self.grow, self.feather, "StillRegions")
        for name in ("pin", "composite"):
            if not isinstance(getattr(self, name), bool):
                raise ValueError(f"StillRegions: {name} {getattr(self, name)!r}: True or False")


def still_map(ends_px, rule=StillRegions()):
    """`ops.still_map` for the keyframe pixels of a batch of clips, `Conditions.ends_px` (b, 3, 2, H, W) with H and W multiples
    of 8 -> (mask (b, 1, 1, H / 8, W / 8) fp32: 1 on the latent positions to hold; alpha (b, H, W) fp32: the pixel weight of the
    keyframes; dist (b, H / 8, W / 8) uint8: cells to the nearest moved cell, capped).  Device tensors, no synchronisation."""
    if not isinstance(rule, StillRegions):
        raise ValueError(f"still_map: rule: expected a StillRegions, got {type(rule).__name__}")
    if not isinstance(ends_px, torch.Tensor) or ends_px.dim() != 5 or ends_px.shape[1:3] != (3, 2):
        raise ValueError(f"still_map: ends_px must be (b, 3, 2, H, W), got {tuple(getattr(ends_px, 'shape', ()))}")
    return ops.still_map(ends_px.to(torch.float32).contiguous(), tau=rule.tau, grow=rule.grow, feather=rule.feather)


def still_pins(cond, mask, t):
    """The pair for `sample(..., pinned=...)` that holds the still cells of `still_map`'s `mask` (b, 1, 1, h, w): x0 (b, 4, t, h,
    w) with x0[:, :, j] = z0 + s_j (z1 - z0), s_j = float32(j) / float32(t - 1), z0 and z1 frames 0 and t - 1 of `cond.endpoints`
    (the latents the conditions already hold: no further encoder call), and the mask broadcast over t, (b, 1, t, h, w)."""
    z, t = cond.endpoints, int(t)
    if z is None or z.dim() != 5 or z.shape[2] != t or t < 2:
        raise ValueError(f"still_pins: conditions with endpoint latents of {t} >= 2 frames, got "
                         f"{None if z is None else tuple(z.shape)}")
    if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (z.shape[0], 1, 1, *z.shape[3:]):
        raise ValueError(f"still_pins: mask must be {(z.shape[0], 1, 1, *z.shape[3:])}, got {tuple(getattr(mask, 'shape', ()))}")
    z0, z1 = z[:, :, 0].to(torch.float32).unsqueeze(2), z[:, :, t - 1].to(torch.float32).unsqueeze(2)
    s = (torch.arange(t, dtype=torch.float32, device=z.device) / torch.tensor(float(t - 1), dtype=torch.float32, device=z.device))
    x0 = z0 + s.view(1, 1, t, 1, 1) * (z1 - z0)
    return x0, mask.to(torch.float32).expand(-1, -1, t, -1, -1).contiguous()


def join_pins(frames, regions):
    """One (x0, mask) pair of whole pinned frames (`pin_frames`: mask (b, 1, t, 1, 1)) and still regions (`still_pins`: mask
    (b, 1, t, h, w)): the masks combine by maximum, and where a whole frame is pinned its own x0 wins.  Either may be None."""
    if frames is None or regions is None:
        return regions if frames is None else frames
    (xf, mf), (xr, mr) = frames, regions
    whole = mf.to(device=mr.device, dtype=torch.float32)
    return torch.where(whole > 0, xf.to(device=xr.device, dtype=torch.float32), xr), torch.maximum(whole.expand_as(mr), mr)


def _check_still(what, still, hold_endpoints=True):
    if still is None:
        return
    if not isinstance(still, StillRegions):
        raise ValueError(f"{what}: still: expected a StillRegions, got {type(still).__name__}")
    if not hold_endpoints:
        raise ValueError(f"{what}: still= without hold_endpoints: both keyframe slots hold the same frame, everything would be still")


def _still_plan(cond, still, t, pinned=None):
    """(pinned, alpha) of a batch of clips under `still` (None: `pinned` as it is, no alpha and no call): its map from the batch's
    own keyframes, the still cells joined to `pinned` with `still.pin`, the pixel weight with `still.composite`."""
    if still is None or not (still.pin or still.composite):
        return pinned, None
    mask, alpha, _ = still_map(cond.ends_px, still)
    if still.pin:
        pinned = join_pins(pinned, still_pins(cond, mask, t))
    return pinned, alpha if still.composite else None


def sample(model, cond: Conditions, plan: SamplingPlan, latent_shape, x_T=None, pinned=None, variant=0):
    """Latents (b, 4, t, h, w) of one clip batch.  `pinned`: an (x0, mask) pair (`pin_frames`) -- where mask is one the
    latent is held at x0, noised to each step's level, while the rest is sampled (the reference's `mask` / `x0`).  As there,
    the returned latents are not blended once more: pinned frames come out close to x0, not equal to it.  With `plan.seeds`
    (or `seeds` among `plan.extra`) clip i draws from `variant_seed(seeds[i], variant)`.  `plan.order` (or `solver_order` among
    `plan.extra`) goes to the sampler as `solver_order`."""
    check_frames(latent_shape[2])
    sampler = (ThreeWaySampler if cond.three_way else DDIMSampler)(model)
    extra = dict(plan.extra)
    x_T = extra.pop("x_T", x_T)                    # the reference's callers hand the start noise over among their **kwargs
    x0, mask = pinned if pinned is not None else (None, None)
    x0, mask = extra.pop("x0", x0), extra.pop("mask", mask)       # ... and `mask` / `x0` likewise
    seeds = extra.pop("seeds", plan.seeds)
    order = extra.pop("solver_order", plan.order)
    if seeds is not None:
        seeds = [variant_seed(s, variant) for s in ops.clip_seeds(seeds, latent_shape[0], "sample: seeds")]
    out, _ = sampler.sample(S=plan.steps, conditioning=cond.positive, batch_size=latent_shape[0], shape=tuple(latent_shape[1:]),
                            verbose=False, unconditional_guidance_scale=plan.scale, unconditional_conditioning=cond.negative,
                            eta=plan.eta, cfg_img=plan.image_scale, mask=mask, x0=x0, fs=cond.fs,
                            timestep_spacing=plan.spacing, guidance_rescale=plan.rescale, x_T=x_T,
                            unconditional_conditioning_img_nonetext=cond.image_only, seeds=seeds, solver_order=order,
                            **extra)
    return out


def decode_spliced(model, latents, refs, marks=None):
    """Decode all T frames; decode again without frames 1 and T-2 (the endpoints' neighbours) and let that second pass's two
    centre frames replace the first pass's (the reference's anti-flicker step, inference.py:262-268).  `marks`: optional
    callable invoked between the passes (bench.py records HIP events there)."""
    t = latents.shape[2]
    video = model.decode_first_stage(latents, ref_context=refs)
    if marks is not None:
        marks()
    keep = [i for i in range(t) if i not in (1, t - 2)]
    again = model.decode_first_stage(latents[:, :, keep].contiguous(), ref_context=refs)
    c = t // 2
    video[:, :, c - 1:c + 1] = again[:, :, c - 2:c]
    return video


def _cond_options(plan, three_way, hold_endpoints, prompts, fs):
    """The keyword options of `Conditions.build` / `from_uint8` / `from_planes` that a synthesis call makes of its own"""
    return dict(prompts=prompts, fs=fs, guided=plan.scale != 1.0, three_way=three_way, image_branch=plan.image_scale != 1.0,
                hold_endpoints=hold_endpoints)


def _finish(model, cond, plan, latent_shape, *, pinned=None, alpha=None, match=None, pinned_px=None, variant=0):
    """The finishing chain of every synthesis call, in its one order: `sample`, `decode_spliced`, then `match` (an
    `output.ColourMatch`: the decoded clip matched in colour to the keyframes of its conditions, `output.match_colour`; with
    `match.targets == "pinned"` the {frame index: pixels} of `pinned_px` are further targets, its inner), then `alpha`
    (`still_map`'s pixel weight: the still pixels held to the keyframes, `output.hold_still`, in place -- the clip is this
    module's own).  None means no call: without `match` no colour op runs, without `alpha` no still op."""
    video = decode_spliced(model, sample(model, cond, plan, latent_shape, pinned=pinned, variant=variant), cond.refs)
    if match is not None:
        inner = pinned_px and getattr(match, "targets", "ends") == "pinned"
        video = match_colour(video, cond.ends_px, match, inner={int(i): px for i, px in pinned_px.items()} if inner else None)
    if alpha is not None:
        video = hold_still(video, cond.ends_px, alpha, inplace=True)
    return video


def synthesize(model, videos, latent_shape, *, plan: SamplingPlan, prompts=None, fs=24, three_way=False, hold_endpoints=True,
               variants=1, keyframes=None, match=None, still=None):
    """(b, variants, 3, t, H, W) pixels in [-1, 1].  `keyframes`: {frame index: (b, 3, H, W) pixels} held in place between
    the endpoints while the rest is sampled (`pin_frames`; encoded once for all variants).  The concat conditioning stays
    endpoints-only: that is what the model was trained on.  With `plan.seeds`, variant k of clip i is the clip seeded
    `variant_seed(plan.seeds[i], k)`: the same pixels as a `variants=1` run with that seed.
    match: an `output.ColourMatch` -- every decoded clip is matched in colour to frames 0 and t-1 of `videos` (frame 0 alone
    without hold_endpoints) before it is returned, by a linear map ("mkl", "mean_std") or by histogram ("hm", "hm_mkl_hm");
    None: no colour op is called.  `ColourMatch(targets="ends")`, the default: the targets are the two endpoints only, and
    `keyframes=` pins latents without adding targets.  `ColourMatch(targets="pinned")`: every pinned frame is a target too --
    frame i is matched to `keyframes[i]` itself, the one image whose colours are known there, and the frames between two
    targets to the course from one to the next (`match_colour`'s inner).  `ColourMatch(max_gain=g)` limits the linear gains.
    still: a `StillRegions` -- what does not move between frames 0 and t-1 of `videos` is held (one tc_still_map call for all
    variants; H and W multiples of 8).  With `still.pin` the still cells join the sampler's mask, their x0 the course between the
    endpoint latents (`still_pins`); where `keyframes=` pins a whole frame that frame's own x0 and mask win (`join_pins`).  With
    `still.composite` the still pixels of every decoded clip are the keyframes' own, feathered towards the moving area
    (`output.hold_still`), after `match=`.  Needs hold_endpoints (ValueError otherwise).  None: no still op is called.  The
    defaults of `StillRegions` are unmeasured starting values."""
    _check_still("synthesize", still, hold_endpoints)
    cond = Conditions.build(model, videos, **_cond_options(plan, three_way, hold_endpoints, prompts, fs))
    pinned = pin_frames(model, keyframes, latent_shape[2]) if keyframes else None
    pinned, alpha = _still_plan(cond, still, latent_shape[2], pinned)
    return torch.stack([_finish(model, cond, plan, latent_shape, pinned=pinned, alpha=alpha, match=match, pinned_px=keyframes, variant=k)
                        for k in range(variants)], dim=1)


def synthesize_u8(model, first_u8, last_u8, latent_shape, *, size, plan: SamplingPlan, prompts=None, fs=24, three_way=False,
                  hold_endpoints=True, out_size=None, out_filter="bicubic", out_fmt="rgb24", out_colour=None, match=None, still=None):
    """uint8 keyframes in, uint8 clip out, all on the device: (b, h, w, 3) first / last frames -> (b, t, H, W, 3) frames
    (`Conditions.from_uint8`, `sample`, `decode_spliced`, `clip_to_uint8`).  The last frame of one clip can be the first
    keyframe of the next without leaving the GPU.  `plan.seeds` as in `sample`.
    out_size = (oh, ow), out_filter, out_fmt: the delivery size and pixel format (`clip_to_uint8`'s size / filter / fmt, the
    pixel back end) -- (b, t, oh, ow, 3) frames, or for "i420" / "nv12" the (b, t, oh * ow * 3 / 2) planes that
    `mp4.write_mp4_i420` or an encoder takes.  out_colour: an `output.Colour` for those planes (`clip_to_uint8`'s colour).
    match: an `output.ColourMatch` -- the decoded clip is matched in colour to the two keyframes at model size
    (`output.match_colour`; methods "mkl", "mean_std", "hm", "hm_mkl_hm"; `max_gain` as there) before it goes to the writer;
    None: no colour op is called.  This call pins nothing: `targets="pinned"` means "ends" here.
    still: a `StillRegions` -- what does not move between the two keyframes at model size is held, as in `synthesize`: the still
    cells' latents during sampling, the still pixels after `match=` and before the writer.  None: no still op is called."""
    _check_still("synthesize_u8", still, hold_endpoints)
    cond = Conditions.from_uint8(model, first_u8, last_u8, size=size, t=latent_shape[2],
                                 **_cond_options(plan, three_way, hold_endpoints, prompts, fs))
    pinned, alpha = _still_plan(cond, still, latent_shape[2])
    video = _finish(model, cond, plan, latent_shape, pinned=pinned, alpha=alpha, match=match)
    return clip_to_uint8(video, size=out_size, filter=out_filter, fmt=out_fmt, colour=out_colour)


def timeline_layout(keyframes: int, t: int, batch: int, out_hw, fmt: str, colour=None):
    """Where a timeline of `keyframes` keyframes puts its frames (the splice rule of tc_frames_to_u8, include/tooncrafter_hip.h):
    segment i runs from keyframe i to i + 1; segment 0 gives frames 0 .. t-1 of the video, every later one its frames 1 .. t-1,
    F = (K - 1)(t - 1) + 1 frames in all.  Returns (F, bytes per frame, batches); a batch is (first segment, segments) and its
    frames 1 .. t-1 start at video frame first * (t - 1) + 1, clips (t - 1) frames apart.  colour: the `output.Colour` of planar
    frames (fmt "i420" / "nv12"); its bits = 10 ("nv12" only: P010) doubles the bytes per frame."""
    keyframes, t, batch = int(keyframes), int(t), int(batch)
    oh, ow = (int(v) for v in out_hw)
    if keyframes < 2 or t < 2 or batch < 1:
        raise ValueError(f"timeline: {keyframes} keyframes (at least 2), clips of {t} frames (at least 2), batches of {batch}")
    if fmt not in ("rgb24", "i420", "nv12"):
        raise ValueError(f"timeline: out_fmt {fmt!r}: 'rgb24', 'i420' or 'nv12'")
    if oh <= 0 or ow <= 0 or (fmt != "rgb24" and (oh % 2 or ow % 2)):
        raise ValueError(f"timeline: output size {(oh, ow)} for {fmt}")
    if colour is not None and (fmt == "rgb24" or (colour.bits == 10 and fmt != "nv12")):
        raise ValueError(f"timeline: out_fmt {fmt!r} with a {colour.bits}-bit colour: 'i420' or 'nv12', 10 bits 'nv12' only")
    segments = keyframes - 1
    frame = oh * ow * 3 if fmt == "rgb24" else oh * ow * 3 // 2
    if colour is not None and colour.bits == 10:
        frame *= 2
    return segments * (t - 1) + 1, frame, [(i, min(batch, segments - i)) for i in range(0, segments, batch)]


SHOT_LABELS = ("tween", "cut", "hold")


def timeline_segments(labels, segments: int, batch: int, what: str = "timeline_segments"):
    """Which segments of a timeline are held and how the others are sampled, host arithmetic only: `labels` one of SHOT_LABELS
    per segment (None: every segment "tween") -> (held, batches).  held: the segments labelled anything but "tween", in order.
    batches: (first segment, segments) as in `timeline_layout` -- the maximal runs of consecutive "tween" segments, each cut into
    chunks of at most `batch`, so no batch spans a held segment; with None they are `timeline_layout`'s batches.  `what`: the
    caller's name for the ValueError."""
    labels = ("tween",) * segments if labels is None else tuple(labels)
    if len(labels) != segments or any(v not in SHOT_LABELS for v in labels) or batch < 1:
        raise ValueError(f"{what}: labels {labels} for {segments} segments, each one of {SHOT_LABELS}, in batches of {batch}")
    held, batches = [], []
    for i, label in enumerate(labels):
        if label != "tween":
            held.append(i)
        elif batches and sum(batches[-1]) == i and batches[-1][1] < batch:
            batches[-1] = (batches[-1][0], batches[-1][1] + 1)
        else:
            batches.append((i, 1))
    return held, batches


@dataclass(frozen=True)
class ShotRule:
    """What `find_shots` makes of tc_frame_deltas' counts for one segment (keyframe i -> i + 1), S_c the samples of component c:
      moved = sum_c changed_c / sum_c S_c     the share of samples that differ by more than `tau` code values;
      mad   = sum_c sad_c / sum_c S_c         the mean absolute difference in code values;
      hist  = max_c hist_l1_c / (2 S_c)       the largest share of a component's 64-bin histogram that changed place.
    "hold" if moved <= hold_moved; otherwise "cut" if hist >= cut_hist and mad >= cut_mad; otherwise "tween".  The comparisons
    are made in exact rational arithmetic on the thresholds as written (`Fraction(str(v))`), so a tie is a tie.
    The defaults are starting values.  Nobody has measured them on real footage: no claim is made that they find the cuts or
    the holds of any source.  A dissolve or a fade is a gradual change and is not a cut by this rule."""
    tau: int = 8
    hold_moved: float = 0.002
    cut_hist: float = 0.35
    cut_mad: float = 20.0

    def __post_init__(self):
        import numbers
        if isinstance(self.tau, bool) or not isinstance(self.tau, numbers.Integral) or not 0 <= int(self.tau) <= 255:
            raise ValueError(f"ShotRule: tau {self.tau!r}: an integer in [0, 255]")
        for name in ("hold_moved", "cut_hist", "cut_mad"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not 0 <= v < float("inf"):
                raise ValueError(f"ShotRule: {name} {v!r}: a finite number >= 0")


@dataclass(frozen=True)
class ShotPlan:
    """One label per segment of a timeline, "tween" | "cut" | "hold", and -- where `find_shots` made it -- the three measures
    of `ShotRule` per segment as Python floats (None for a plan written by hand: `ShotPlan(("tween", "cut", "tween"))`)."""
    labels: tuple
    moved: Optional[tuple] = None
    mad: Optional[tuple] = None
    hist: Optional[tuple] = None

    def __post_init__(self):
        object.__setattr__(self, "labels", tuple(self.labels))
        bad = [v for v in self.labels if v not in SHOT_LABELS]
        if bad:
            raise ValueError(f"ShotPlan: label {bad[0]!r}: one of {SHOT_LABELS}")

    def distinct(self):
        """The keyframe indices that begin a new drawing: 0, and i + 1 for every segment i that is not a hold."""
        return [0] + [i + 1 for i, label in enumerate(self.labels) if label != "hold"]


def frame_deltas(keyframes, lag=1, tau=8):
    """`ops.frame_deltas` for the keyframes of a timeline: (K, h, w, 3) uint8 or a `Planes` of K images -> (delta (K - lag, 3, 3)
    int64: sad, changed, hist_l1 per pair (i, i + lag) and component; hist (K, 3, 64) int32), device tensors, exact integers,
    no synchronisation (tc_frame_deltas)."""
    _check_images("frame_deltas: keyframes", keyframes, "K", planes=True)
    return ops.frame_deltas(keyframes, lag=lag, tau=tau)


def component_samples(keyframes):
    """Samples per component of one keyframe: (h w, h w, h w) for RGB frames, (h w, ch cw, ch cw) for a `Planes`."""
    if isinstance(keyframes, Planes):
        h, w = keyframes.y.shape[1:3]
        return (h * w, ((h + 1) // 2) * ((w + 1) // 2), ((h + 1) // 2) * ((w + 1) // 2))
    h, w = keyframes.shape[1:3]
    return (h * w,) * 3


def label_shots(table, samples, rule=ShotRule()):
    """The `ShotPlan` of a (K - 1, 3, 3) table of integers (sad, changed, hist_l1 per segment and component) over `samples`
    = (S_0, S_1, S_2): `ShotRule`'s labels, every comparison cross-multiplied in Python integers and fractions.  Host only."""
    from fractions import Fraction
    s = [int(v) for v in samples]
    if len(s) != 3 or min(s) <= 0:
        raise ValueError(f"label_shots: samples {samples}: three positive counts")
    hold, cut_hist, cut_mad = (Fraction(str(v)) for v in (rule.hold_moved, rule.cut_hist, rule.cut_mad))
    total = sum(s)
    labels, moved, mad, hist = [], [], [], []
    for row in table:
        row = [[int(v) for v in comp] for comp in row]
        if len(row) != 3 or any(len(comp) != 3 for comp in row):
            raise ValueError("label_shots: the table must be (segments, 3, 3)")
        m = Fraction(sum(comp[1] for comp in row), total)
        d = Fraction(sum(comp[0] for comp in row), total)
        q = max(Fraction(comp[2], 2 * sc) for comp, sc in zip(row, s))
        labels.append("hold" if m <= hold else "cut" if q >= cut_hist and d >= cut_mad else "tween")
        moved.append(float(m))
        mad.append(float(d))
        hist.append(float(q))
    return ShotPlan(tuple(labels), tuple(moved), tuple(mad), tuple(hist))


def find_shots(keyframes, rule=ShotRule()):
    """Where a timeline should not interpolate: one tc_frame_deltas call (lag 1, tau = rule.tau) over the K keyframes, then ONE
    device-to-host copy of its (K - 1, 3, 3) table -- that copy waits for the device: a synchronisation, so this call cannot be
    captured in a graph -- and `label_shots` on the host.  Returns the `ShotPlan`.  The default rule's thresholds are unmeasured
    starting values (`ShotRule`)."""
    if not isinstance(rule, ShotRule):
        raise ValueError(f"find_shots: rule: expected a ShotRule, got {type(rule).__name__}")
    delta, _ = frame_deltas(keyframes, lag=1, tau=rule.tau)
    return label_shots(delta.cpu().tolist(), component_samples(keyframes), rule)


def synthesize_timeline_u8(model, keyframes, latent_shape, *, size, plan: SamplingPlan, prompts=None, fs=24, three_way=False,
                           out_size=None, out_filter="bicubic", out_fmt="rgb24", out_colour=None, match=None, shots=None, still=None):
    """K keyframes in, one video out, all on the device.  `keyframes`: (K, h, w, 3) uint8 or a `Planes` of K images, K >= 2.
    Segment i interpolates keyframe i -> i + 1 (endpoints held); segments run in order, latent_shape[0] per batch (the last
    batch may be smaller), each batch exactly `Conditions.from_uint8` / `from_planes` with first = kf[i : i + n] and
    last = kf[i + 1 : i + n + 1], `sample`, `decode_spliced` and tc_frames_to_u8 writing into ONE buffer by `timeline_layout`'s
    rule: (F, oh, ow, 3) for "rgb24", (F, oh * ow * 3 / 2) for "i420" / "nv12" (what `mp4.write_mp4_i420` / `planar_writer`
    take), F = (K - 1)(t - 1) + 1.  `plan.seeds`: one seed per SEGMENT (sliced per batch); `prompts`: one per segment or None.
    Without seeds the device generator is drawn as the same sequence of `synthesize_u8` calls draws it.  Every inner keyframe is
    encoded twice, as one segment's last frame and the next one's first.
    out_colour: an `output.Colour` for planar frames (tc_frames_to_yuv instead; 10 bits: (F, oh * ow * 3) bytes of P010), or
    "source": the colour the `Planes` keyframes came in (`Colour.of`), so the video leaves in the description it arrived with.
    match: an `output.ColourMatch` -- every batch of segments is matched in colour to its own keyframes (`output.match_colour`)
    before it is written: the last frame of segment i and frame 0 of segment i + 1 then have the same target, the inner
    keyframe's statistics ("mkl", "mean_std") or its per-channel quantile function ("hm", "hm_mkl_hm"), so the video does not
    step in colour there.  `max_gain` as in `match_colour`; a timeline pins nothing, so `targets="pinned"` means "ends" here.
    None: no colour op is called.
    shots: None -- every segment is sampled, the calls are exactly those above; a `ShotPlan` (K - 1 labels), or a `ShotRule`, which
    runs `find_shots` on the keyframes first (one synchronising copy of a small table).  A segment labelled "cut" or "hold" is
    not sampled: its frames 1 .. t-2 are keyframe i and its frame t-1 is keyframe i + 1 (frame 0 too is keyframe 0 for segment
    0), each the bytes that the front end (`frames_from_uint8` / `frames_from_planes` at `size`) followed by the writer gives
    for that keyframe; no colour match is applied to them, they are the targets.  The length and layout stay
    `timeline_layout`'s.  Sampled segments are batched as maximal runs of consecutive "tween" segments, each run cut into chunks
    of latent_shape[0]: a batch never spans a skipped segment, and every chunk is the `synthesize_u8` call it replaces.
    `plan.seeds` and `prompts` stay indexed by the original segment number.  The default rule's thresholds are unmeasured.
    still: a `StillRegions` -- every batch of sampled segments holds what does not move between its own keyframe pairs (one
    tc_still_map call per batch, at model size; `synthesize_u8`'s still): the still cells' latents during sampling, the still
    pixels after `match=` and before the writer.  "cut" and "hold" segments are untouched.  None: no still op is called."""
    _check_still("synthesize_timeline_u8", still)
    _check_images("synthesize_timeline_u8: keyframes", keyframes, "K", planes=True)
    planar = isinstance(keyframes, Planes)
    k, t = len(keyframes), int(latent_shape[2])
    size = tuple(int(v) for v in size)
    oh, ow = size if out_size is None else (int(v) for v in out_size)
    if out_colour is not None and not isinstance(out_colour, (str, Colour)):
        raise ValueError(f"synthesize_timeline_u8: out_colour: expected a Colour or 'source', got {type(out_colour).__name__}")
    if isinstance(out_colour, str):
        if out_colour != "source" or not planar:
            raise ValueError(f"synthesize_timeline_u8: out_colour {out_colour!r}: a Colour, or 'source' with Planes keyframes "
                             "(RGB keyframes carry no colour description)")
        out_colour = Colour.of(keyframes)
    total, frame, _ = timeline_layout(k, t, latent_shape[0], (oh, ow), out_fmt, out_colour)
    seeds = None if plan.seeds is None else ops.clip_seeds(plan.seeds, k - 1, "synthesize_timeline_u8: plan.seeds (one per segment)")
    if prompts is not None and len(prompts) != k - 1:
        raise ValueError(f"synthesize_timeline_u8: {len(prompts)} prompts for {k - 1} segments")
    if isinstance(shots, ShotRule):
        shots = find_shots(keyframes, shots)
    if shots is not None and not isinstance(shots, ShotPlan):
        raise ValueError(f"synthesize_timeline_u8: shots: expected a ShotRule or a ShotPlan, got {type(shots).__name__}")
    held, batches = timeline_segments(None if shots is None else shots.labels, k - 1, latent_shape[0], "synthesize_timeline_u8: shots")
    video = torch.empty((total, oh, ow, 3) if out_fmt == "rgb24" else (total, frame), dtype=torch.uint8,
                        device=keyframes.y.device if planar else keyframes.device)
    wide = out_colour is not None and out_colour.bits == 10                                       # P010: 2-byte samples
    flat, row = video.view(-1), 3 * ow if out_fmt == "rgb24" else 2 * ow if wide else ow
    how = dict(size=out_size, filter=out_filter, fmt=out_fmt, colour=out_colour)

    def put(i, clips):
        """`clips`, the segments from i on, into the video: frame 0 if segment 0 is among them, frames 1 .. t-1 at their place"""
        if i == 0:
            write_frames(clips[:1], frames=(0, 1), out=flat, strides=(row, frame, frame), **how)
        write_frames(clips, frames=(1, t - 1), out=flat[(i * (t - 1) + 1) * frame:], strides=(row, frame, (t - 1) * frame), **how)
    build, front = (Conditions.from_planes, frames_from_planes) if planar else (Conditions.from_uint8, frames_from_uint8)
    for i in held:                                    # not sampled: t - 1 frames of keyframe i, then keyframe i + 1, as the writer gives them
        ends = front(keyframes[i:i + 2], size, [(0, 0), (0, 1)], 2)
        put(i, ends[:, :, [0] * (t - 1) + [1]].contiguous())
    for i, n in batches:
        cond = build(model, keyframes[i:i + n], keyframes[i + 1:i + n + 1], size=size, t=t,
                     **_cond_options(plan, three_way, True, None if prompts is None else list(prompts[i:i + n]), fs))
        part = plan if seeds is None else replace(plan, seeds=seeds[i:i + n])
        pinned, alpha = _still_plan(cond, still, t)
        put(i, _finish(model, cond, part, [n, *latent_shape[1:]], pinned=pinned, alpha=alpha, match=match).to(torch.float32))
    return video


# --- the reference scripts' call signatures (scripts/evaluation/inference.py:164,180) -----------------------------------

def get_latent_z_with_hidden_states(model, videos):
    z0, z1, refs = encode_endpoints(model, videos)
    b, t = videos.shape[0], videos.shape[2]
    z = z0.new_zeros((b, z0.shape[1], t, *z0.shape[2:]))
    z[:, :, 0], z[:, :, t - 1] = z0, z1
    return z, refs


def image_guided_synthesis(model, prompts, videos, noise_shape, n_samples=1, ddim_steps=50, ddim_eta=1.,
                           unconditional_guidance_scale=1.0, cfg_img=None, fs=None, text_input=False,
                           multiple_cond_cfg=False, loop=False, interp=False, timestep_spacing='uniform',
                           guidance_rescale=0.0, solver_order=1, match=None, **kwargs):
    """`solver_order` and `match` are not in the reference's signature (a script that never passes them gets the reference's
    sampler and frames): 2 switches the multistep correction on, `SamplingPlan.order`; an `output.ColourMatch` matches the
    decoded clips in colour to the keyframes (`synthesize`'s match)."""
    plan = SamplingPlan(steps=ddim_steps, eta=ddim_eta, scale=unconditional_guidance_scale, image_scale=cfg_img,
                        spacing=timestep_spacing, rescale=guidance_rescale, extra=kwargs, order=solver_order)
    return synthesize(model, videos, noise_shape, plan=plan, prompts=prompts if text_input else None, fs=fs,
                      three_way=multiple_cond_cfg, hold_endpoints=bool(loop or interp), variants=n_samples, match=match)
