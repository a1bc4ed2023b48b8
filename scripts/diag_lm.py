#!/usr/bin/env python3
"""AWD-LSTM decode step, kernel by kernel (V=60000, reference dims): each op of the step
captured alone 50x into one graph and replayed back to back, then the whole step, so the
per-kernel time is measured without the profiler (and with the weights of only that op cycling
through the caches vs the whole step's 181 MB). Prints one JSON document."""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipzap import _native as N  # noqa: E402
from hipzap.engine.lm import LMEngine  # noqa: E402
from hipzap.models.awd_lstm import reference_lm  # noqa: E402


def timed(build, reps=50, iters=20):
    lib = N.lib()
    s = torch.cuda.Stream()
    prog = lib.hz_prog_create()
    for _ in range(reps):
        build(prog)
    N.check(lib.hz_prog_capture(prog, s.cuda_stream), "capture")
    P = (C.c_void_p * 1)(prog)
    S = (C.c_void_p * 1)(s.cuda_stream)
    out = (C.c_double * 2)()
    N.check(lib.hz_prog_bench2(P, S, 1, 3, 0, out), "warm")
    N.check(lib.hz_prog_bench2(P, S, 1, iters, 0, out), "bench")
    lib.hz_prog_destroy(prog)
    return round(out[1] / iters / reps, 3)


def main():
    V = int(os.environ.get("HIPZAP_LM_VOCAB", 60000))
    torch.manual_seed(0)
    eng = LMEngine.from_state_dict(reference_lm(V).state_dict(), "cuda:0", unroll=1)
    eng.run_tokens([1, 2], 4, 0)
    lib = N.lib()
    ops = eng._ops  # (kind, params) in step order; the sampler is fused into layer 0
    res_final = None if eng._final is None else \
        timed(lambda p: N.prog_add(lib, p, N.HZ_K_SAMPLER, eng._final, 0, "final"))
    res = {"V": V, "standalone_argmax_sampler_us": res_final}
    for k, (kind, prm) in enumerate(ops):
        name = lib.hz_kernel_name(kind).decode()[len("HZ_K_"):].lower()  # lstm, decoder, sampler
        res[f"{k}_{name}_us"] = timed(
            lambda p, kind=kind, prm=prm, name=name: N.prog_add(lib, p, kind, prm, 0, name))

    def step(p):
        for kind, prm in ops:
            N.prog_add(lib, p, kind, prm, 0, "step")
        N.prog_add(lib, p, N.HZ_K_STEP_BUMP, N.StepBumpArgs(eng.step.data_ptr(), 1), 0, "bump")
    res["step_us"] = timed(step, reps=8)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
