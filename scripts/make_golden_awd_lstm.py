#!/usr/bin/env python3
"""Record the reference AWD-LSTM module's weights and eval outputs for tests/test_awd_lstm_cpu.py.

    python scripts/make_golden_awd_lstm.py PATH/TO/pytorch_models/awd_lstm.py

Writes tests/golden/awd_lstm_ref.npz (unidirectional, 5 stateful steps) and
tests/golden/awd_lstm_ref_bidir.npz (one forward): ``sd/<key>`` = the reference's random-init
state_dict, ``x`` = the token batches, ``y`` = its decoded outputs. Data only: the tests load the
weights into hipzap's own module and compare against ``y``."""
import importlib.util
import os
import sys

import numpy as np
import torch

KW = dict(vocab_sz=120, emb_sz=40, n_hid=48, n_layers=3, pad_token=1, tie_weights=True, bias=True, qrnn=False)
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def main():
    spec = importlib.util.spec_from_file_location("ref_awd_lstm", sys.argv[1])
    ref_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_mod)
    os.makedirs(OUT, exist_ok=True)
    for name, kw, shapes in (("awd_lstm_ref", KW, [(3, 2)] * 5), ("awd_lstm_ref_bidir", dict(KW, bidir=True), [(7, 3)])):
        torch.manual_seed(0)
        ref = ref_mod.get_language_model(**kw).eval()
        ref.reset()
        xs = [torch.randint(0, KW["vocab_sz"], s) for s in shapes]
        with torch.no_grad():
            ys = [ref(x)[0] for x in xs]
        arrays = {f"sd/{k}": v.numpy() for k, v in ref.state_dict().items()}
        np.savez_compressed(os.path.join(OUT, f"{name}.npz"), x=torch.stack(xs).numpy(), y=torch.stack(ys).numpy(),
                            **arrays)


if __name__ == "__main__":
    main()
