"""Vector search over the embeddings this runtime produces: ``.hzidx`` index files, the GPU
:class:`Index` (csrc/index.cpp + csrc/search.hip) and the fp64 oracle :func:`search_ref`.

torch-free, like :mod:`hipzap.lite`: numpy and ctypes only.

File format ``.hzidx`` (version 1): ``HzIndexHeader`` (csrc/hipzap.h: magic, version, the JSON header's
length, the row block's offset, count, dim, metric), the JSON header ``{"dim", "count", "dtype": "bf16",
"metric": "cosine" | "ip", "model", "embed": {"pooling", "normalize", "dim"} | null, "labels"?}``, zero
padding, then the bf16 rows ``[count][dim]`` at a 4096-aligned offset.

Order rule (kernels and oracle alike): higher score first; among equal scores the lower row id first;
``-0.0`` counts as ``+0.0``; with fewer than ``k`` rows the slots past ``count`` hold id -1, score -inf.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import queue
import struct

import numpy as np

from .ops.search import MAX_K, MAX_Q

MAGIC = b"HZIDX\0\0\1"
VERSION = 1
METRICS = ("cosine", "ip")
ALIGN = 4096
HEAD = struct.Struct("<8sIIQQII")  # HzIndexHeader: magic, version, json_len, data_off, count, dim, metric


def to_bf16(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 bit patterns (uint16), round to nearest even; the input must be finite."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def write_index(path: str, vectors, metric: str = "cosine", labels=None, model: str = "", embed=None) -> dict:
    """Write ``vectors`` (fp32 [N, D]) as a ``.hzidx`` file and return its JSON header. ``cosine`` rows are
    divided by max(||v||, 1e-12) in fp32 and then rounded to bf16; ``ip`` rows are only rounded."""
    v = np.asarray(vectors)
    if v.ndim != 2 or v.dtype.kind != "f":
        raise ValueError(f"vectors must be a float array [N, D], got {v.dtype} {list(v.shape)}")
    v = np.ascontiguousarray(v, np.float32)
    n, d = v.shape
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    if d < 8 or d % 8 or d > 2048:
        raise ValueError(f"dim must be a multiple of 8 in 8..2048, got {d}")
    if n < 1 or n >= 2 ** 31:
        raise ValueError(f"count must be in 1..2^31-1, got {n}")
    bad = np.flatnonzero(~np.isfinite(v).all(axis=1))
    if bad.size:
        raise ValueError(f"row {int(bad[0])} has a non-finite value ({bad.size} such rows)")
    if labels is not None:
        labels = [str(s) for s in labels]
        if len(labels) != n:
            raise ValueError(f"{len(labels)} labels for {n} rows")
    if metric == "cosine":
        norm = np.sqrt((v * v).sum(axis=1, dtype=np.float32), dtype=np.float32)
        v = v / np.maximum(norm, np.float32(1e-12))[:, None]
    rows = to_bf16(v)
    if not np.isfinite(bf16_to_f32(rows)).all():
        raise ValueError("a value overflows bf16")
    hdr = {"dim": d, "count": n, "dtype": "bf16", "metric": metric, "model": str(model or ""),
           "embed": dict(embed) if embed else None}
    if labels is not None:
        hdr["labels"] = labels
    js = json.dumps(hdr).encode()
    data_off = -(-(HEAD.size + len(js)) // ALIGN) * ALIGN
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(HEAD.pack(MAGIC, VERSION, len(js), data_off, n, d, METRICS.index(metric)))
        f.write(js)
        f.write(bytes(data_off - HEAD.size - len(js)))
        f.write(rows.tobytes())
    os.replace(tmp, path)
    return hdr


def read_header(path: str) -> dict:
    """The JSON header of a ``.hzidx`` file, checked against the fixed head; plus ``data_off``."""
    with open(path, "rb") as f:
        raw = f.read(HEAD.size)
        if len(raw) < HEAD.size or raw[:8] != MAGIC:
            raise ValueError(f"{path} is not a .hzidx file")
        _, version, json_len, data_off, count, dim, metric = HEAD.unpack(raw)
        if version != VERSION:
            raise ValueError(f"{path}: unknown .hzidx version {version}")
        hdr = json.loads(f.read(json_len))
    if metric >= len(METRICS) or (hdr.get("dim"), hdr.get("count"), hdr.get("metric")) != (dim, count, METRICS[metric]) \
            or hdr.get("dtype") != "bf16":
        raise ValueError(f"{path}: the JSON header disagrees with the file head")
    if hdr.get("labels") is not None and len(hdr["labels"]) != count:
        raise ValueError(f"{path}: {len(hdr['labels'])} labels for {count} rows")
    return dict(hdr, data_off=int(data_off))


def read_rows(path: str) -> np.ndarray:
    """The row block as bf16 bit patterns, uint16 [count, dim]."""
    hdr = read_header(path)
    return np.fromfile(path, np.uint16, hdr["count"] * hdr["dim"], offset=hdr["data_off"]).reshape(hdr["count"], hdr["dim"])


def search_ref(corpus, q, k: int):
    """The oracle: ``corpus`` (the bf16 rows widened to fp32, [N, D]) against ``q`` (fp32 [Q, D]) in fp64
    -> (scores float64 [Q, k], ids int32 [Q, k]) under the order rule. Each score is one row's own sum, so
    equal rows give equal scores wherever they stand."""
    c = np.asarray(corpus, np.float64)
    q = np.asarray(q, np.float64)
    if q.ndim == 1:
        q = q[None]
    n = c.shape[0]
    scores = np.full((q.shape[0], k), -np.inf)
    ids = np.full((q.shape[0], k), -1, np.int32)
    for i, row in enumerate(q):
        s = (c * row[None, :]).sum(axis=1) + 0.0  # -0.0 + 0.0 = +0.0
        order = np.argsort(-s, kind="stable")[:k]  # stable: equal scores keep ascending ids
        scores[i, :order.size] = s[order]
        ids[i, :order.size] = order
    return scores, ids


def check_queries(q, dim: int) -> np.ndarray:
    q = np.asarray(q)
    if q.ndim == 1:
        q = q[None]
    if q.ndim != 2 or q.shape[1] != dim:
        raise ValueError(f"query vectors must be [Q, {dim}], got {list(q.shape)}")
    q = np.ascontiguousarray(q, np.float32)
    if not np.isfinite(q).all():
        raise ValueError("a query vector has a non-finite value")
    return q


def check_k(k) -> int:
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise ValueError(f"k must be an integer in 1..{MAX_K}, got {k!r}")
    return int(k)


def normalize_rows(q: np.ndarray) -> np.ndarray:
    """q / max(||q||, 1e-12) per row in fp32 (what a cosine index expects of its queries)."""
    q = np.asarray(q, np.float32)
    norm = np.sqrt((q * q).sum(axis=1, dtype=np.float32), dtype=np.float32)
    return q / np.maximum(norm, np.float32(1e-12))[:, None]


class _Base:
    def __init__(self, path: str):
        self.path = path
        self.header = read_header(path)
        self.dim, self.count, self.metric = self.header["dim"], self.header["count"], self.header["metric"]
        self.labels = self.header.get("labels")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class RefIndex(_Base):
    """The index on the host: :func:`search_ref` over the file's rows (the CPU backend's implementation)."""
    backend = "cpu"

    def __init__(self, path: str):
        super().__init__(path)
        self._rows = bf16_to_f32(read_rows(path))

    def search(self, q, k: int = 10):
        q, k = check_queries(q, self.dim), check_k(k)
        s, i = search_ref(self._rows, q, k)
        return s.astype(np.float32), i

    def describe(self) -> dict:
        return {"path": self.path, "backend": "cpu", **{k: v for k, v in self.header.items() if k != "labels"},
                "labels": self.labels is not None}

    def close(self) -> None:
        self._rows = None


class Index(_Base):
    """An open ``.hzidx`` on the GPU: the rows in device memory and ``contexts`` search contexts (each
    its own stream and buffers). :meth:`search` is thread-safe: a call takes a free context, or waits for
    one. Query batches above 16 rows are searched 16 at a time."""
    backend = "gpu"

    def __init__(self, path: str, device: int = 0, contexts: int = 2):
        super().__init__(path)
        from . import _native as N
        self._lib = N.lib()
        self._h = self._lib.hz_index_open(os.fsencode(path), int(device), int(contexts))
        if not self._h:
            raise RuntimeError((self._lib.hz_index_last_error() or b"hz_index_open failed").decode())
        self.device, self.contexts = int(device), int(contexts)
        self._free: queue.Queue = queue.Queue()
        for c in range(self.contexts):
            self._free.put(c)

    def search(self, q, k: int = 10, ctx: int | None = None):
        """fp32 queries [Q, dim] -> (scores float32 [Q, k], ids int32 [Q, k]), best first."""
        q, k = check_queries(q, self.dim), check_k(k)
        if self._h is None:
            raise RuntimeError("the index is closed")
        scores = np.empty((q.shape[0], k), np.float32)
        ids = np.empty((q.shape[0], k), np.int32)
        c = self._free.get() if ctx is None else ctx
        try:
            for a in range(0, q.shape[0], MAX_Q):
                part = q[a:a + MAX_Q]
                s, i = scores[a:a + MAX_Q], ids[a:a + MAX_Q]  # contiguous row ranges of the outputs
                rc = self._lib.hz_index_search(self._h, c, part.ctypes.data, part.shape[0], k, s.ctypes.data, i.ctypes.data)
                if rc:
                    raise RuntimeError(f"hz_index_search failed with code {rc}")
        finally:
            if ctx is None:
                self._free.put(c)
        return scores, ids

    def describe(self) -> dict:
        out = (C.c_uint64 * 8)()
        self._lib.hz_index_describe(self._h, out)
        return {"path": self.path, "backend": "gpu", "device": self.device,
                **{k: v for k, v in self.header.items() if k != "labels"}, "labels": self.labels is not None,
                "contexts": int(out[3]), "tile_rows": int(out[4]), "programs": int(out[5]), "device_bytes": int(out[6])}

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.hz_index_close(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def open_index(path: str, backend: str = "gpu", device: int = 0):
    return Index(path, device) if backend == "gpu" else RefIndex(path)
