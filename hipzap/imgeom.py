"""Resize + centre-crop geometry of the resize plans, torch-free (``hipzap/lite.py`` serves without
torch). The ONE definition every layer shares: host validation, the fp32 oracle
(``ops/vision.py resize_preprocess_reference``, which re-exports these) and the header the kernel
reads (``csrc/vision.hip resize_preprocess_kernel``)."""
from __future__ import annotations


def resize_geometry(H: int, W: int, resize: int = 256, crop: int = 224) -> tuple[int, int, int, int]:
    """(rh, rw, top, left) of torchvision's ``Resize(resize)`` + ``CenterCrop(crop)`` on an H x W image:
    the shorter side becomes ``resize`` (the longer one truncated), the crop origin is rounded half to
    even (Python ``round``)."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"image size {H}x{W}")
    if H <= W:
        rh, rw = resize, (resize * W) // H
    else:
        rh, rw = (resize * H) // W, resize
    return rh, rw, int(round((rh - crop) / 2.0)), int(round((rw - crop) / 2.0))


def resize_cap_bytes(max_h: int, max_w: int) -> int:
    """Bytes per request row of a resize plan's image input: max_h * max_w * 3 rounded up to 16."""
    return (int(max_h) * int(max_w) * 3 + 15) // 16 * 16


def resize_dims(H: int, W: int, resize: int = 256, crop: int = 224, max_h: int | None = None,
                max_w: int | None = None) -> list[int]:
    """The kernel's per-image header {H, W, rh, rw, top, left, 0, 0}, validated against the plan's
    maximum (the error names the limit)."""
    H, W = int(H), int(W)
    if max_h is not None and (H > max_h or W > max_w):
        raise ValueError(f"image {H}x{W} exceeds this plan's maximum of {max_h}x{max_w} (height x width)")
    if resize < crop:
        raise ValueError(f"resize {resize} < crop {crop}: the crop would leave the resized image")
    return [H, W, *resize_geometry(H, W, resize, crop), 0, 0]


def parse_max_image(s) -> tuple[int, int]:
    """``"1024x768"`` (height x width), ``"1024"`` or a pair -> (max_h, max_w)."""
    if isinstance(s, (list, tuple)):
        h, w = s
    else:
        parts = str(s).lower().split("x")
        h, w = (parts[0], parts[0]) if len(parts) == 1 else parts
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"max image {s!r}")
    return h, w


def resize_spec(resize, crop: int = 224, max_image=None) -> tuple[int, int, int, int] | None:
    """(resize, crop, max_h, max_w) from the settings / CLI values (``resize`` None or 0: no resize
    plan); the maximum defaults to 1024 x 1024."""
    if not resize:
        return None
    mh, mw = parse_max_image(max_image or (1024, 1024))
    resize, crop = int(resize), int(crop)
    if resize < crop:
        raise ValueError(f"resize {resize} < crop {crop}")
    return resize, crop, mh, mw
