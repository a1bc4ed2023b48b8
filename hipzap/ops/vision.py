"""Eager wrappers + fp32 oracles for the vision helper kernels (csrc/vision.hip)."""
from __future__ import annotations

import ctypes as C

import torch

from .. import _native as N
from ..imgeom import resize_cap_bytes, resize_dims, resize_geometry  # noqa: F401  (the shared, torch-free geometry)

K_POOL_FC = N.HZ_K_POOL_FC


@N.params_of("HZ_K_POOL_FC")
class PoolFcParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p), ("B", C.c_int),
                ("C", C.c_int), ("HW", C.c_int), ("N", C.c_int), ("ldo", C.c_int),
                ("pooled", C.c_int), ("pad_", C.c_int)]


@N.params_of("HZ_K_POOL_NORM")
class PoolNormParams(C.Structure):  # HzPoolNormParams (csrc/hipzap.h)
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("B", C.c_int), ("C", C.c_int), ("HW", C.c_int),
                ("ldo", C.c_int), ("pooled", C.c_int), ("normalize", C.c_int)]


@N.params_of("HZ_K_AVGPOOL")
class AvgpoolArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("N", C.c_int), ("HW", C.c_int), ("C", C.c_int),
                ("blocked", C.c_int)]


@N.params_of("HZ_K_PREPROCESS")
class PreprocessArgs(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("mean", C.c_void_p), ("inv_std", C.c_void_p),
                ("N", C.c_int), ("Cin", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Cpad", C.c_int),
                ("mode", C.c_int)]


@N.params_of("HZ_K_RESIZE_PATCHIFY")  # the same block; ``out`` is then the ViT patch rows
@N.params_of("HZ_K_RESIZE_PREPROCESS")
class ResizeParams(C.Structure):
    _fields_ = [("image", C.c_void_p), ("dims", C.c_void_p), ("out", C.c_void_p), ("B", C.c_int), ("crop", C.c_int),
                ("maxH", C.c_int), ("maxW", C.c_int), ("cap_bytes", C.c_longlong), ("mean", C.c_float * 4),
                ("inv_std", C.c_float * 4)]


IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


# ---------------------------------------------------------------- resize + centre crop + normalise
def resize_preprocess_reference(img_u8: torch.Tensor, mean=IMAGENET_MEAN, std=IMAGENET_STD, resize: int = 256,
                                crop: int = 224, cpad: int = 8) -> torch.Tensor:
    """fp32 oracle of the resize kernel: one uint8 [H, W, 3] image -> [crop, crop, cpad] float32.
    Antialiased bilinear resize of the float image on the CPU, centre crop, / 255, (x - mean) / std,
    channels zero-padded to ``cpad``."""
    img = torch.as_tensor(img_u8)
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[-1] == 3, tuple(img.shape)
    H, W = img.shape[:2]
    rh, rw, top, left = resize_geometry(H, W, resize, crop)
    x = img.cpu().permute(2, 0, 1).float()[None]
    y = torch.nn.functional.interpolate(x, size=(rh, rw), mode="bilinear", antialias=True, align_corners=False)
    y = y[0, :, top: top + crop, left: left + crop].permute(1, 2, 0) / 255.0
    if mean is not None:
        y = (y - torch.tensor(mean, dtype=torch.float32)) / torch.tensor(std, dtype=torch.float32)
    return torch.nn.functional.pad(y, (0, cpad - 3))


def resize_params(image_ptr: int, dims_ptr: int, out_ptr: int, batch: int, crop: int, max_h: int, max_w: int,
                  mean=None, std=None) -> ResizeParams:
    """Bound HzResizeParams; the normalisation constants are the standalone preprocess kernel's
    (inv_std = 1 / std in fp32)."""
    prm = ResizeParams(image_ptr, dims_ptr, out_ptr, batch, crop, max_h, max_w, resize_cap_bytes(max_h, max_w))
    mu = torch.tensor(mean if mean is not None else (0.0, 0.0, 0.0), dtype=torch.float32)
    inv = 1.0 / torch.tensor(std if std is not None else (1.0, 1.0, 1.0), dtype=torch.float32)
    for c in range(3):
        prm.mean[c], prm.inv_std[c] = float(mu[c]), float(inv[c])
    prm.inv_std[3] = 1.0
    return prm


def pack_images(images, resize: int, crop: int, max_h: int, max_w: int, batch: int | None = None):
    """uint8 [H, W, 3] images (tensors or arrays, any sizes within the maximum) -> the resize plan's two
    request inputs on the host: ``image`` [B, cap_bytes] uint8 with each image packed at its row's
    start, ``dims`` [B, 8] int32. Rows beyond ``len(images)`` repeat the last header over an unwritten
    row (a partial batch)."""
    imgs = [torch.as_tensor(im) for im in images]
    b = batch or len(imgs)
    if not 1 <= len(imgs) <= b:
        raise ValueError(f"{len(imgs)} images for a batch of {b}")
    buf = torch.zeros(b, resize_cap_bytes(max_h, max_w), dtype=torch.uint8)
    dims = torch.zeros(b, 8, dtype=torch.int32)
    for i in range(b):
        im = imgs[min(i, len(imgs) - 1)]
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[-1] != 3:
            raise ValueError(f"an image is uint8 [H, W, 3], got {im.dtype} {tuple(im.shape)}")
        dims[i] = torch.tensor(resize_dims(im.shape[0], im.shape[1], resize, crop, max_h, max_w), dtype=torch.int32)
        if i < len(imgs):
            buf[i, : im.numel()] = im.reshape(-1)
    return buf, dims


def resize_preprocess(image: torch.Tensor, dims: torch.Tensor, crop: int, max_h: int, max_w: int, mean=None,
                      std=None) -> torch.Tensor:
    """Eager launch of the resize kernel: ``image`` [B, cap_bytes] uint8 and ``dims`` [B, 8] int32 on
    the device (or pinned host memory) -> bf16 [B, crop, crop, 8]."""
    b = image.shape[0]
    assert image.dtype == torch.uint8 and image.shape == (b, resize_cap_bytes(max_h, max_w)), tuple(image.shape)
    assert dims.dtype == torch.int32 and dims.shape == (b, 8) and image.is_contiguous() and dims.is_contiguous()
    dev = image.device if image.is_cuda else torch.device("cuda", torch.cuda.current_device())
    out = torch.empty(b, crop, crop, 8, device=dev, dtype=torch.bfloat16)
    prm = resize_params(image.data_ptr(), dims.data_ptr(), out.data_ptr(), b, crop, max_h, max_w, mean, std)
    N.check(N.lib().hz_launch_kernel(N.HZ_K_RESIZE_PREPROCESS, C.byref(prm), N.stream_ptr()), "resize_preprocess")
    return out


def resize_patchify(image: torch.Tensor, dims: torch.Tensor, crop: int, max_h: int, max_w: int, mean=None,
                    std=None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Eager launch of the resize + patchify kernel: the inputs of ``resize_preprocess`` -> bf16 ViT patch
    rows [B * (crop/16)^2, 768], columns in (c, ky, kx) order (``patchify``'s layout). ``out``: a
    contiguous bf16 tensor of that many elements to write into (default: a fresh one)."""
    b = image.shape[0]
    assert image.dtype == torch.uint8 and image.shape == (b, resize_cap_bytes(max_h, max_w)), tuple(image.shape)
    assert dims.dtype == torch.int32 and dims.shape == (b, 8) and image.is_contiguous() and dims.is_contiguous()
    dev = image.device if image.is_cuda else torch.device("cuda", torch.cuda.current_device())
    rows = b * (crop // 16) ** 2
    if out is None:
        out = torch.empty(rows, 768, device=dev, dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.numel() == rows * 768 and out.is_cuda
    prm = resize_params(image.data_ptr(), dims.data_ptr(), out.data_ptr(), b, crop, max_h, max_w, mean, std)
    N.check(N.lib().hz_launch_kernel(N.HZ_K_RESIZE_PATCHIFY, C.byref(prm), N.stream_ptr()), "resize_patchify")
    return out


def resize_patchify_reference(images, mean=IMAGENET_MEAN, std=IMAGENET_STD, resize: int = 256, crop: int = 224,
                              patch: int = 16) -> torch.Tensor:
    """fp32 oracle of ``resize_patchify``: uint8 [H, W, 3] images -> float32 [B * (crop/patch)^2,
    3 * patch * patch]: ``resize_preprocess_reference`` per image, then the patchify rearrangement."""
    x = torch.stack([resize_preprocess_reference(im, mean, std, resize, crop, cpad=3) for im in images])
    b, n = x.shape[0], crop // patch
    x = x.permute(0, 3, 1, 2).reshape(b, 3, n, patch, n, patch).permute(0, 2, 4, 1, 3, 5)
    return x.reshape(b * n * n, 3 * patch * patch).contiguous()


def maxpool_nhwc(x: torch.Tensor, k=3, stride=2, pad=1) -> torch.Tensor:
    n, h, w, c = x.shape
    p = (h + 2 * pad - k) // stride + 1
    q = (w + 2 * pad - k) // stride + 1
    out = torch.empty(n, p, q, c, device=x.device, dtype=torch.bfloat16)
    prm = N.PoolParams(x.data_ptr(), out.data_ptr(), n, h, w, c, p, q, k, stride, pad)
    N.check(N.lib().hz_maxpool_launch(prm, N.stream_ptr()), "maxpool")
    return out


def avgpool_nhwc(x: torch.Tensor, blocked: bool = False) -> torch.Tensor:
    """x: logical [N,H,W,C]; ``blocked`` stores it channel-blocked on device first."""
    from .conv import to_blocked
    n, h, w, c = x.shape
    src = to_blocked(x) if blocked else x.contiguous()
    out = torch.empty(n, c, device=x.device, dtype=torch.bfloat16)
    N.check(N.lib().hz_avgpool_launch(src.data_ptr(), out.data_ptr(), n, h * w, c, int(blocked), N.stream_ptr()),
            "avgpool")
    return out


def pool_fc(x: torch.Tensor, pc, blocked_input: bool = False) -> torch.Tensor:
    """Fused global-average-pool + Linear: x logical [B,H,W,C] bf16 -> fp32 logits [B, cout]."""
    from .conv import to_blocked
    b, h, w, c = x.shape
    assert c == pc.K == pc.ksteps * 32 and c % 32 == 0
    src = x if blocked_input else to_blocked(x)
    out = torch.empty(b, pc.cout, device=x.device, dtype=torch.float32)
    prm = PoolFcParams(src.data_ptr(), pc.wf.data_ptr(), pc.bias.data_ptr(), out.data_ptr(), b, c, h * w, pc.cout,
                       pc.cout)
    N.check(N.lib().hz_launch_kernel(K_POOL_FC, C.byref(prm), N.stream_ptr()), "pool_fc")
    return out


def pool_fc_ref(x: torch.Tensor, pc) -> torch.Tensor:
    """fp32 oracle: x logical [B,H,W,C]."""
    pooled = x.float().mean(dim=(1, 2))
    return pooled @ pc.dense().float().t() + pc.bias.float()


def pool_norm(x: torch.Tensor, normalize: bool = True, blocked_input: bool = False,
              out: torch.Tensor | None = None) -> torch.Tensor:
    """Global average pool [+ L2 normalisation] (csrc/vision.hip pool_norm_kernel): x logical [B,H,W,C]
    bf16 (``blocked_input``: ``ops.conv.to_blocked``'s [B, C/32, H, W, 32] already) -> fp32 [B, C]; an fp32
    [B, C] ``x`` is taken as the channel means a tail seam wrote (``pooled``). ``out``: an fp32 [B, >= C]
    tensor to write into (columns past C are left alone; the returned view is its first C columns)."""
    from .conv import to_blocked
    pooled = x.dtype == torch.float32
    if pooled:
        b, c = x.shape
        hw, src = 1, x.contiguous()
    elif blocked_input:
        b, cb, h, w, c32 = x.shape
        assert c32 == 32 and x.is_contiguous(), tuple(x.shape)
        c, hw, src = cb * 32, h * w, x
    else:
        b, h, w, c = x.shape
        assert c % 32 == 0, c
        hw, src = h * w, to_blocked(x)
    if out is None:
        out = torch.empty(b, c, device=x.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.shape[0] == b and out.stride(1) == 1
    prm = PoolNormParams(src.data_ptr(), out.data_ptr(), b, c, hw, out.stride(0), int(pooled), int(bool(normalize)))
    N.check(N.lib().hz_launch_kernel(N.HZ_K_POOL_NORM, C.byref(prm), N.stream_ptr()), "pool_norm")
    return out[:, :c]


def pool_norm_ref(x: torch.Tensor, normalize: bool = True) -> torch.Tensor:
    """fp64 oracle: x logical [B,H,W,C] (or [B, C] channel means) -> [B, C] float64; ``normalize`` divides
    by max(||row||, 1e-12)."""
    v = x.double()
    if v.dim() == 4:
        v = v.mean(dim=(1, 2))
    if normalize:
        v = v / v.norm(dim=1, keepdim=True).clamp(min=1e-12)
    return v


def preprocess(src: torch.Tensor, cpad: int = 8, mean=None, std=None) -> torch.Tensor:
    """fp32 NCHW (mode 0) or uint8 NHWC (mode 1) -> bf16 NHWC with ``cpad`` channels."""
    if src.dtype == torch.uint8:
        n, h, w, cin = src.shape
        mode = 1
    else:
        n, cin, h, w = src.shape
        mode = 0
    out = torch.empty(n, h, w, cpad, device=src.device, dtype=torch.bfloat16)
    mean_t = inv_t = None
    if mean is not None:
        mean_t = torch.tensor(mean, dtype=torch.float32, device=src.device)
        inv_t = 1.0 / torch.tensor(std, dtype=torch.float32, device=src.device)
    N.check(N.lib().hz_preprocess_launch(src.data_ptr(), out.data_ptr(), n, cin, h, w, cpad, mode,
                                         N.ptr(mean_t), N.ptr(inv_t), N.stream_ptr()), "preprocess")
    return out


def patchify(src: torch.Tensor, patch: int = 16, mean=None, std=None) -> torch.Tensor:
    """fp32 NCHW -> bf16 patch rows [N*(H/P)*(W/P)][C*P*P], columns in (c, ky, kx) order (preprocess
    mode 2, csrc/vision.hip patchify_kernel: the ViT patch embedding's GEMM operand)."""
    n, cin, h, w = src.shape
    out = torch.empty(n * (h // patch) * (w // patch), cin * patch * patch, device=src.device, dtype=torch.bfloat16)
    mean_t = inv_t = None
    if mean is not None:
        mean_t = torch.tensor(mean, dtype=torch.float32, device=src.device)
        inv_t = 1.0 / torch.tensor(std, dtype=torch.float32, device=src.device)
    N.check(N.lib().hz_preprocess_launch(src.data_ptr(), out.data_ptr(), n, cin, h, w, patch, 2,
                                         N.ptr(mean_t), N.ptr(inv_t), N.stream_ptr()), "patchify")
    return out


def patchify_reference(src: torch.Tensor, patch: int = 16) -> torch.Tensor:
    n, c, h, w = src.shape
    x = src.float().reshape(n, c, h // patch, patch, w // patch, patch).permute(0, 2, 4, 1, 3, 5)
    return x.reshape(n * (h // patch) * (w // patch), c * patch * patch).to(torch.bfloat16)


def preprocess_reference(src: torch.Tensor, cpad: int = 8, mean=None, std=None) -> torch.Tensor:
    if src.dtype == torch.uint8:
        x = src.float() / 255.0
    else:
        x = src.float().permute(0, 2, 3, 1)
    if mean is not None:
        x = (x - torch.tensor(mean, device=x.device)) / torch.tensor(std, device=x.device)
    return torch.nn.functional.pad(x, (0, cpad - x.shape[-1]))
