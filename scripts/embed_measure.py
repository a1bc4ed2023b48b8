#!/usr/bin/env python3
"""The two measurements of profiles/embed/README.md on one MI355X, as JSON lines.

1. ``pool_embed_kernel`` alone against the same pooling written as torch ops (bf16 hidden states ->
   fp32 masked mean -> L2 normalise), at (B16, L128, D768, masked mean) and (B64, L197, D768, first=1):
   rounds alternate the two, each round times ``--launches`` back-to-back launches with device events.
2. BERT-base bs16 L128 end to end: the embedding engine against the classification engine of the same
   checkpoint shape, ``--pairs`` interleaved pairs of ``Engine.bench`` (captured replays, one context)."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipzap.engine.engine import Engine  # noqa: E402
from hipzap.models import bert  # noqa: E402
from hipzap.ops import transformer as T  # noqa: E402

DEV = "cuda:0"


def _opt(flag, default):
    return int(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


def _time(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per launch


def kernel(B, L, D, first, masked, rounds, launches):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B * L, D, generator=g).to(torch.bfloat16).to(DEV)
    on = torch.ones(B, L)
    if masked:
        for b in range(B):
            on[b, 16 + (37 * b) % (L - 16):] = 0
    on[:, :first] = 0
    mask = ((1 - on) * -1e9).to(DEV) if masked else None
    on_d = on.to(DEV)
    out = torch.empty(B, D, device=DEV)

    def hip():
        T.pool_embed(x, B, L, mask, "mean", first, True, out=out)

    def ops():
        v = (x.view(B, L, D).float() * on_d[:, :, None]).sum(1) / on_d.sum(1, keepdim=True).clamp(min=1e-9)
        return torch.nn.functional.normalize(v, dim=1)

    hip()
    torch.cuda.synchronize()
    assert (ops() - out).abs().max() < 1e-5  # the same transform
    hs, ts = [], []
    for _ in range(rounds):
        hs.append(_time(hip, launches))
        ts.append(_time(ops, launches))
    return {"what": "kernel", "B": B, "L": L, "D": D, "first": first, "masked": masked, "rounds": rounds,
            "launches_per_round": launches, "hip_us": [round(v, 2) for v in hs], "torch_ops_us": [round(v, 2) for v in ts],
            "hip_us_median": round(statistics.median(hs), 2), "torch_ops_us_median": round(statistics.median(ts), 2)}


def end_to_end(pairs, iters):
    torch.manual_seed(0)
    sd = bert.make_model(2).state_dict()
    B, L = 16, 128
    cls = Engine.from_state_dict("bert-base", sd, DEV, batch=B, arch_kw={"seq_len": L})
    emb = Engine.from_state_dict("bert-base", sd, DEV, batch=B,
                                 arch_kw={"seq_len": L, "head": "embed", "pooling": "mean", "normalize": True})
    for e in (cls, emb):
        e.bench(20)
    c, m = [], []
    for _ in range(pairs):
        c.append(B * iters / cls.bench(iters))
        m.append(B * iters / emb.bench(iters))
    ratios = [b / a for a, b in zip(c, m)]
    return {"what": "bert-base bs16 L128, 1 context, captured replays", "pairs": pairs, "iters": iters,
            "ops": {"classification": cls.contexts[0].num_ops(), "embedding": emb.contexts[0].num_ops()},
            "classification_seq_s": [round(v, 1) for v in c], "embedding_seq_s": [round(v, 1) for v in m],
            "embedding_over_classification": [round(r, 4) for r in ratios],
            "ratio_median": round(statistics.median(ratios), 4),
            "pair_to_pair_spread": round((max(ratios) - min(ratios)), 4)}


def main():
    rounds, launches = _opt("--rounds", 7), _opt("--launches", 200)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__}), flush=True)
    print(json.dumps(kernel(16, 128, 768, 0, True, rounds, launches)), flush=True)
    print(json.dumps(kernel(64, 197, 768, 1, False, rounds, launches)), flush=True)
    print(json.dumps(end_to_end(_opt("--pairs", 5), _opt("--iters", 100))), flush=True)


if __name__ == "__main__":
    main()
