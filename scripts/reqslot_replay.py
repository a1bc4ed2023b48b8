#!/usr/bin/env python3
"""ResNet-50 bs=1 uint8 request program replayed back to back on ONE stream, for kernel traces of
the request path (profiles/reqslot): ``rocprofv3 --kernel-trace --stats -- python
scripts/reqslot_replay.py [dev|host] [iters]``. ``dev``: device-resident request slot + the one-launch
stem (28 launches); ``host``: pinned request + preprocess + convpool (29 launches).

``python scripts/reqslot_replay.py copy`` prints the host cost of one 150,528-byte payload copy
instead: memcpy into pinned memory against the streaming copy into a device slot, 1 and 12 threads."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def copy_cost():
    import torch
    from hipzap import _native as N
    torch.cuda.init()
    n, threads = 150528, 12
    src = torch.randint(0, 256, (n + 3,), dtype=torch.uint8)
    dev = [N.reqslot_alloc(n) for _ in range(threads)]
    assert all(s and s[2] == N.REQSLOT_DEVICE for s in dev), "no host-writable device memory"
    pin = [torch.zeros(n, dtype=torch.uint8).pin_memory() for _ in range(threads)]
    out = (C.c_double * 2)()
    V = C.c_void_p * threads
    for name, slots, streaming in (("memcpy -> pinned host", V(*[p.data_ptr() for p in pin]), 0),
                                   ("streaming copy -> device slot", V(*[s[1] for s in dev]), 1),
                                   ("memcpy -> device slot", V(*[s[1] for s in dev]), 0)):
        for t in (1, threads):
            N.check(N.lib().hz_reqslot_copy_bench(slots, src.data_ptr() + 3, n, t, 2000, streaming, out), "copy_bench")
            print(f"{name:32s} threads={t:2d}  best {out[0]:7.2f} us  median {out[1]:7.2f} us", flush=True)
    for s in dev:
        N.reqslot_free(s[0], s[2])


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "dev"
    if mode == "copy":
        return copy_cost()
    os.environ["HIPZAP_REQSLOT"] = mode
    import torch
    from hipzap.engine.engine import Engine
    from hipzap.models import registry
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    a = registry.get("resnet50")
    torch.manual_seed(0)
    params, arch_kw = a.pack(a.make_model().eval().state_dict(), "cuda:0")
    eng = Engine("resnet50", params, "cuda:0", batch=1, num_contexts=1, arch_kw=dict(arch_kw, input_uint8=True),
                 host_io=True, zero_copy="all")
    c = eng.contexts[0]
    c.write_input(0, torch.randint(0, 256, tuple(c.host_input.shape), dtype=torch.uint8))
    eng.bench(20)
    t = eng.bench(iters)
    print(f"{mode}: {c.num_ops()} launches, first {[f.kind for f in c.fused.values()][0]}, "
          f"{iters} replays, {t / iters * 1e6:.1f} us each", flush=True)


if __name__ == "__main__":
    main()
