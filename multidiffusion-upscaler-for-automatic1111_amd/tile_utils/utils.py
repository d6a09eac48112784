"""
Tile utilities of the plugin surface (same public names as upstream tile_utils/utils.py), with every map / grid
computation routed through the mdtile engine (libmdtile.so, include/mdtile.h):

    split_bboxes      upstream utils.py:160-177  -> mdtile_plan_create + mdtile_weight_map_add_grid
    gaussian_weights  upstream utils.py:180-194  -> mdtile_gaussian_weights
    feather_mask      upstream utils.py:196-214  -> mdtile_feather_mask
    get_retouch_mask  upstream utils.py:216-247  -> mdtile_retouch_mask (upstream: OpenCV box filters on the CPU; no OpenCV here)
    upscale_init_image  the host's Upscaler.upscale as scripts/tilediffusion.py:141-147 calls it -> mdtile_resample_u8 for its Pillow resizes
    color_fix_image   nothing upstream (StableSR's wavelet / AdaIN colour fix, CPU code of another extension) -> mdtile_colorfix_wavelet,
                      mdtile_hist_u8 + mdtile_lut_u8; opt-in, --mdtile-color-fix

Prompt / cond helpers stay thin host-side Python (they only forward to `modules.prompt_parser`).
"""
from __future__ import annotations

import math
import os
from collections import namedtuple
from enum import Enum
from typing import Any, Dict, List, Optional, Tuple, Union

import torch
from torch import Tensor

from modules import devices, shared
from modules.processing import opt_f

import mdtile


class ComparableEnum(Enum):
    def __eq__(self, other: Any) -> bool:
        if isinstance(other, str):
            return self.value == other
        if isinstance(other, ComparableEnum):
            return self.value == other.value
        raise TypeError(f"unsupported type: {type(other)}")

    __hash__ = Enum.__hash__


class Method(ComparableEnum):
    MULTI_DIFF = "MultiDiffusion"
    MIX_DIFF = "Mixture of Diffusers"


class Method_2(ComparableEnum):
    DEMO_FU = "DemoFusion"


class BlendMode(Enum):
    FOREGROUND = "Foreground"
    BACKGROUND = "Background"


# field order == the 10 gradio controls of one region block == upstream BBoxSettings (utils.py:41)
BBoxSettings = namedtuple("BBoxSettings", ["enable", "x", "y", "w", "h", "prompt", "neg_prompt", "blend_mode",
                                           "feather_ratio", "seed"])
NoiseInverseCache = namedtuple("NoiseInversionCache", ["model_hash", "x0", "xt", "noise_inversion_steps", "retouch", "prompts"])
DEFAULT_BBOX_SETTINGS = BBoxSettings(False, 0.4, 0.4, 0.2, 0.2, "", "", BlendMode.BACKGROUND.value, 0.2, -1)
NUM_BBOX_PARAMS = len(BBoxSettings._fields)


def build_bbox_settings(bbox_control_states: List[Any]) -> Dict[int, BBoxSettings]:
    """Positional gradio values -> {region index: settings}; floats rounded to 4 digits, disabled / degenerate regions
    dropped (upstream utils.py:47-63)."""
    out: Dict[int, BBoxSettings] = {}
    for index, start in enumerate(range(0, len(bbox_control_states), NUM_BBOX_PARAMS)):
        s = BBoxSettings(*bbox_control_states[start:start + NUM_BBOX_PARAMS])
        s = s._replace(x=round(s.x, 4), y=round(s.y, 4), w=round(s.w, 4), h=round(s.h, 4),
                       feather_ratio=round(s.feather_ratio, 4), seed=int(s.seed))
        if s.enable and s.x <= 1.0 and s.y <= 1.0 and s.w > 0.0 and s.h > 0.0:
            out[index] = s
    return out


def gr_value(value=None, visible=None):
    return {"value": value, "visible": visible, "__type__": "update"}


class BBox:
    """Grid tile rectangle in latent pixels; `slicer` indexes an NCHW tensor."""

    def __init__(self, x: int, y: int, w: int, h: int):
        self.x, self.y, self.w, self.h = x, y, w, h
        self.box = [x, y, x + w, y + h]
        self.slicer = (slice(None), slice(None), slice(y, y + h), slice(x, x + w))

    def __getitem__(self, idx: int) -> int:
        return self.box[idx]

    def __repr__(self):
        return f"{type(self).__name__}(x={self.x}, y={self.y}, w={self.w}, h={self.h})"


def region_rect(fx: float, fy: float, fw: float, fh: float, W: int, H: int, wrap_x: bool = False, wrap_y: bool = False) -> Tuple[int, int, int, int]:
    """(x, y, w, h) in latent pixels of a region given as fractions of a W x H canvas -- the one rule for region rectangles.
    An axis that does not wrap: the origin max(0, int(f * extent)), the size ceil(fs * extent) clipped at the edge (upstream's rule).
    An axis that wraps (--mdtile-wrap-regions on a closed canvas): the origin int(f * extent) mod extent, the size min(extent, ceil(fs * extent));
    the region covers the coordinates (origin + i) mod extent, i in [0, size), so origin + size may pass the extent."""
    def axis(f0: float, fs: float, extent: int, wraps: bool) -> Tuple[int, int]:
        if wraps:
            return int(f0 * extent) % extent, min(extent, math.ceil(fs * extent))
        origin = max(0, int(f0 * extent))
        return origin, min(extent - origin, math.ceil(fs * extent))
    (x, w), (y, h) = axis(fx, fw, W, wrap_x), axis(fy, fh, H, wrap_y)
    return x, y, w, h


class CustomBBox(BBox):
    """Region-prompt rectangle.  Foreground regions carry their feather mask (built on the GPU by the engine).
    cover: a mask region's coverage, dense uint8 [h, w] on the device (the rectangle is the mask's bounding box), with its feather from
    mdtile.mask_region for a foreground region; None: the region is its whole rectangle."""

    def __init__(self, x: int, y: int, w: int, h: int, prompt: str, neg_prompt: str, blend_mode: str,
                 feather_radio: float, seed: int, cover: Optional[Tensor] = None, feather: Optional[Tensor] = None):
        super().__init__(x, y, w, h)
        self.prompt, self.neg_prompt = prompt, neg_prompt
        self.blend_mode = BlendMode(blend_mode)
        self.feather_ratio = max(min(feather_radio, 1.0), 0.0)
        self.seed = seed
        self.cover = cover
        self.index: Optional[int] = None      # the region's key in the job's bbox_settings (init_custom_bbox sets it)
        if self.blend_mode != BlendMode.FOREGROUND:
            self.feather_mask = None
        else:
            self.feather_mask = feather if cover is not None else feather_mask(w, h, self.feather_ratio)
        self.cond = None
        self.extra_network_data = None
        self.uncond = None


def region_mask_sources(p, indices) -> Dict[int, Tuple[Any, str]]:
    """{region index (0-based): (a PIL image or a file path, the name recorded in the generation parameters)} of the regions that are painted
    masks: p.mdtile_region_masks = {k: PIL image or path} with k the 1-based region number, else DIR/region<k>.png of --mdtile-region-masks DIR.
    The attribute wins over the directory."""
    given = getattr(p, "mdtile_region_masks", None) or {}
    folder = getattr(shared.cmd_opts, "mdtile_region_masks", None)
    out: Dict[int, Tuple[Any, str]] = {}
    for i in indices:
        k = i + 1
        src = given.get(k, given.get(str(k)))
        if src is not None:
            out[i] = (src, os.path.basename(src) if isinstance(src, (str, os.PathLike)) else "<image>")
        elif folder:
            path = os.path.join(folder, f"region{k}.png")
            if os.path.isfile(path):
                out[i] = (path, os.path.basename(path))
    return out


def load_region_mask(src) -> Tensor:
    """A region's painted mask as uint8 [Hm, Wm] on the device: the image (or the file, read with Pillow) converted to "L"."""
    import numpy as np
    from PIL import Image
    if isinstance(src, (str, os.PathLike)):
        with Image.open(src) as img:
            a = np.array(img.convert("L"), dtype=np.uint8)
    else:
        a = np.array(src.convert("L"), dtype=np.uint8)
    return torch.from_numpy(a).to(devices.device)


class Prompt:
    @staticmethod
    def apply_styles(prompts: List[str], styles=None) -> List[str]:
        if not styles:
            return prompts
        return [shared.prompt_styles.apply_styles_to_prompt(p, styles) for p in prompts]

    @staticmethod
    def append_prompt(prompts: List[str], prompt: str = "") -> List[str]:
        if not prompt:
            return prompts
        return [f"{p}, {prompt}" for p in prompts]


class Condition:
    """Thin forwards to the host's prompt parser (host-coupled, no arithmetic)."""

    @staticmethod
    def get_custom_cond(prompts: List[str], prompt, steps: int, styles=None):
        from modules import extra_networks
        prompt = Prompt.apply_styles([prompt], styles)[0]
        _, extra_network_data = extra_networks.parse_prompts([prompt])
        prompts = Prompt.apply_styles(Prompt.append_prompt(prompts, prompt), styles)
        return Condition.get_cond(prompts, steps), extra_network_data

    @staticmethod
    def get_cond(prompts, steps: int):
        from modules import extra_networks, prompt_parser
        prompts, _ = extra_networks.parse_prompts(prompts)
        return prompt_parser.get_multicond_learned_conditioning(shared.sd_model, prompts, steps)

    @staticmethod
    def get_uncond(neg_prompts: List[str], steps: int, styles=None):
        from modules import prompt_parser
        return prompt_parser.get_learned_conditioning(shared.sd_model, Prompt.apply_styles(neg_prompts, styles), steps)

    @staticmethod
    def reconstruct_cond(cond, step: int) -> Tensor:
        from modules import prompt_parser
        _, tensor = prompt_parser.reconstruct_multicond_batch(cond, step)
        return tensor

    @staticmethod
    def reconstruct_uncond(uncond, step: int) -> Tensor:
        from modules import prompt_parser
        return prompt_parser.reconstruct_cond_batch(uncond, step)


def splitable(w: int, h: int, tile_w: int, tile_h: int, overlap: int = 16) -> bool:
    """More than one tile for an IMAGE-space canvas (w, h)?  (upstream utils.py:151-158)"""
    w, h = w // opt_f, h // opt_f
    m = min(tile_w, tile_h)
    if overlap >= m:
        overlap = m - 4
    return math.ceil((w - overlap) / (tile_w - overlap)) > 1 or math.ceil((h - overlap) / (tile_h - overlap)) > 1


def split_bboxes(w: int, h: int, tile_w: int, tile_h: int, overlap: int = 16,
                 init_weight: Union[Tensor, float] = 1.0) -> Tuple[List[BBox], Tensor]:
    """Overlapping tile grid + its summed weight map, computed by the engine (raw grid, no clamping)."""
    plan = mdtile.Plan(w, h, tile_w, tile_h, overlap, 1, clamp=False)
    weight = torch.zeros((1, 1, h, w), device=devices.device, dtype=torch.float32)
    tile_w_map = None
    if isinstance(init_weight, Tensor):
        tile_w_map = init_weight.to(device=devices.device, dtype=torch.float32).contiguous()
        mdtile.weight_map_add_grid(plan, tile_w_map, weight)
    else:
        mdtile.weight_map_add_grid(plan, None, weight)
        if float(init_weight) != 1.0:
            weight *= float(init_weight)
    return [BBox(*b) for b in plan.bboxes], weight


def grid_shift(seed: int, step: int, axis: int, extent: int) -> int:
    """--mdtile-grid-shift: the cyclic displacement of the wrapped tile grid along one axis (0 = x, 1 = y) at one sampler step, in
    [0, extent).  A pure integer function (the splitmix64 finaliser on seed + golden-ratio increments): it touches no torch or numpy
    generator, so the sampler's noise does not depend on whether the option is set."""
    m = (1 << 64) - 1
    z = (int(seed) + 0x9E3779B97F4A7C15 * (2 * int(step) + int(axis) + 1)) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z ^= z >> 31
    return z % int(extent)


def lattice_shift(seed: int, step: int, axis: int, stride: int) -> int:
    """--mdtile-grid-jitter: the shift of the jittered grid along one axis (0 = x, 1 = y) at one sampler step, in [1, stride] (stride = the lattice
    at rest).  grid_shift's integers moved up by one: no torch or numpy generator is touched."""
    return 1 + grid_shift(seed, step, axis, stride)


def shifted_bboxes(batched_bboxes: List[List[BBox]], sx: int, sy: int, w: int, h: int) -> List[List[BBox]]:
    """The boxes of a wrap plan with every origin displaced cyclically: ((x + sx) mod w, (y + sy) mod h), same sizes, same order."""
    return [[BBox((b.x + sx) % w, (b.y + sy) % h, b.w, b.h) for b in batch] for batch in batched_bboxes]


def gaussian_weights(tile_w: int, tile_h: int) -> Tensor:
    """Mixture-of-Diffusers tile weight (upstream utils.py:180-194), generated on the GPU in fp64 -> fp32."""
    return mdtile.gaussian_weights(tile_w, tile_h, devices.device)


def feather_mask(w: int, h: int, ratio: float) -> Tensor:
    """Foreground feather mask (upstream utils.py:196-214), generated on the GPU."""
    return mdtile.feather_mask(w, h, ratio, devices.device)


NoiseInverseCache = namedtuple("NoiseInversionCache", ["model_hash", "x0", "xt", "noise_inversion_steps", "retouch", "prompts"])


def get_retouch_mask(img_input, kernel_size: int) -> Tensor:
    """Where an image carries detail: the residue of a self-guided box filter (guided filter with guide = input, eps 0.01), as
    uint8-quantised fractions in [0, 1] float32 (upstream tile_utils/utils.py:216-247), computed on the GPU by mdtile_retouch_mask
    (include/mdtile.h defines the result exactly).  img_input: numpy uint8 array [H, W] (grey) or [H, W, 3] (RGB, converted
    with PIL's "L" formula on the GPU), or such a tensor already on the device.  Returns a TENSOR [H, W] on devices.device where upstream
    returns an ndarray."""
    if not isinstance(img_input, Tensor):
        import warnings
        import numpy as np
        arr = np.ascontiguousarray(img_input)
        if arr.dtype != np.uint8:
            raise TypeError(f"get_retouch_mask: image bytes expected, got dtype {arr.dtype}")
        with warnings.catch_warnings():     # np.asarray(PIL image) is read-only; it is only read here, and copying 200 MB to say so is waste
            warnings.simplefilter("ignore", UserWarning)
            img_input = torch.from_numpy(arr)
    return mdtile.retouch_mask(img_input.to(devices.device).contiguous(), int(round(kernel_size)))


# the host's two resampling upscalers, by the name they are listed under AND the class behind it (an extension may reuse a name)
ENGINE_UPSCALERS = {("Lanczos", "UpscalerLanczos"): mdtile.RESAMPLE_LANCZOS, ("Nearest", "UpscalerNearest"): mdtile.RESAMPLE_NEAREST}


def image_to_device(image) -> Tensor:
    """The bytes of an "RGB" / "L" PIL image as a uint8 tensor [H, W, 3] / [H, W] on devices.device."""
    import warnings
    import numpy as np
    with warnings.catch_warnings():     # np.asarray(PIL image) is read-only; it is only read here
        warnings.simplefilter("ignore", UserWarning)
        return torch.from_numpy(np.asarray(image)).to(devices.device)


def image_from_device(t: Tensor):
    """uint8 [H, W, 3] / [H, W] on the device -> PIL image, through one pinned staging buffer (torch keeps it for the next job)."""
    from PIL import Image
    if t.device.type == "cuda":
        host = torch.empty(t.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(t, non_blocking=True)
        torch.cuda.current_stream(t.device).synchronize()
    else:
        host = t
    return Image.fromarray(host.numpy())


def upscale_init_image(image, upscaler, scale: float) -> Tuple[Any, Optional[Tensor]]:
    """The host's `upscaler.scaler.upscale(image, scale, upscaler.data_path)`, step by step, with every Pillow resize of it on the engine
    (mdtile.resize_u8: the same bytes, include/mdtile.h): the rounds of the built-in Lanczos / Nearest upscalers and the Lanczos fit to the
    multiple of 8 that ends every upscale.  A model upscaler's rounds stay the host's `do_upscale`.  The image goes up once, stays on the
    device between resizes and comes back once.  Returns (PIL image, its bytes on the device or None when the engine did not run); an image
    that is neither "RGB" nor "L", or an upscaler without `do_upscale`, takes the host's call untouched."""
    scaler = upscaler.scaler
    if image.mode not in ("RGB", "L") or not hasattr(scaler, "do_upscale"):
        return scaler.upscale(image, scale, upscaler.data_path), None
    builtin = ENGINE_UPSCALERS.get((upscaler.name, type(scaler).__name__))
    scaler.scale = scale
    dest_w = int(image.width * scale // 8 * 8)
    dest_h = int(image.height * scale // 8 * 8)
    img, t = image, None                # the current image on the host / its bytes on the device: at least one of them is set
    w, h = image.size
    for _ in range(3):
        if w >= dest_w and h >= dest_h:
            break
        before = (w, h)
        if builtin is not None:
            if t is None:
                t = image_to_device(img)
            t, img = mdtile.resize_u8(t, (int(h * scale), int(w * scale)), builtin), None
            w, h = int(t.shape[1]), int(t.shape[0])
        else:
            if img is None:
                img = image_from_device(t)
            img, t = scaler.do_upscale(img, upscaler.data_path), None
            w, h = img.size
        if (w, h) == before:
            break
    if (w, h) != (dest_w, dest_h):
        if t is None and img.mode not in ("RGB", "L"):      # a model that changed the mode: the host's own fit
            from PIL import Image
            lanczos = Image.Resampling.LANCZOS if hasattr(Image, "Resampling") else Image.LANCZOS
            return img.resize((dest_w, dest_h), resample=lanczos), None
        if t is None:
            t = image_to_device(img)
        t, img = mdtile.resize_u8(t, (dest_h, dest_w), mdtile.RESAMPLE_LANCZOS), None
    if img is None:
        img = image_from_device(t)
    return img, t


COLOR_FIX_MODES = ("wavelet", "adain")


def color_fix_image(image, style_image, mode: str, kept=None):
    """The colour fix of --mdtile-color-fix on one finished image: `image` (the decoded result) keeps its detail and takes the low frequencies
    (mode "wavelet") or the per-channel mean and deviation ("adain") of `style_image` (the init image), on bytes as include/mdtile.h defines
    them.  The result goes up once; the style comes from `kept` = (PIL image, its bytes on the device), which Script.process leaves as
    p.init_image_bytes_md, when kept[0] IS style_image, and is uploaded otherwise.  A style of another mode is converted to the result's; one of
    another size is resized with Lanczos on the engine for "wavelet" ("adain" only reads its statistics).  Returns a PIL image; an image that is
    neither "RGB" nor "L" comes back untouched."""
    if mode not in COLOR_FIX_MODES:
        raise ValueError(f"color fix mode {mode!r}: expected one of {COLOR_FIX_MODES}")
    if image.mode not in ("RGB", "L"):
        return image
    content = image_to_device(image)
    if kept is not None and kept[0] is style_image and style_image.mode == image.mode:
        style = kept[1]
    else:
        if style_image.mode != image.mode:
            style_image = style_image.convert(image.mode)
        style = image_to_device(style_image)
    if mode == "adain":
        return image_from_device(mdtile.colorfix_adain(content, style))
    if tuple(style.shape[:2]) != tuple(content.shape[:2]):
        style = mdtile.resize_u8(style, (int(content.shape[0]), int(content.shape[1])), mdtile.RESAMPLE_LANCZOS)
    return image_from_device(mdtile.colorfix_wavelet(content, style))


def null_decorator(fn):
    return fn


keep_signature = controlnet = stablesr = grid_bbox = custom_bbox = noise_inverse = null_decorator
