"""AWD-LSTM: checkpoint compatibility with the reference module, W_hh quirk, stateful API."""
import os

import numpy as np
import pytest
import torch

from hipzap.models.awd_lstm import get_language_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _ref(name):
    """The reference module's recorded run (scripts/make_golden_awd_lstm.py): its random-init
    state_dict, the token batches it was fed and the decoded outputs it returned in eval mode."""
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    return sd, torch.from_numpy(z["x"]), torch.from_numpy(z["y"])


KW = dict(vocab_sz=120, emb_sz=40, n_hid=48, n_layers=3, pad_token=1, tie_weights=True, bias=True, qrnn=False)


def test_state_dict_keys_match_reference():
    ref_sd = _ref("awd_lstm_ref")[0]
    ours = get_language_model(**KW)
    assert set(ref_sd) == set(ours.state_dict())
    for k, v in ref_sd.items():
        assert ours.state_dict()[k].shape == v.shape, k


def test_forward_matches_reference_eval():
    sd, xs, ys = _ref("awd_lstm_ref")
    ours = get_language_model(**KW)
    ours.load_state_dict(sd)
    ours.eval()
    ours.reset()
    assert len(xs) == 5
    for step, (x, a) in enumerate(zip(xs, ys)):
        assert x.shape == (3, 2)
        with torch.no_grad():
            b, rb, ob = ours(x)
        assert a.shape == b.shape == (6, 120)
        assert torch.allclose(a, b, atol=1e-5), step
        assert len(rb) == len(ob) == 3


def test_whh_quirk_module_weight_wins():
    ours = get_language_model(**KW)
    sd = ours.state_dict()
    sd = {k: v.clone() for k, v in sd.items()}
    for l in range(3):
        sd[f"0.rnns.{l}.weight_hh_l0_raw"].zero_()
        sd[f"0.rnns.{l}.module.weight_hh_l0"].fill_(0.5)
    ours.load_state_dict(sd)
    assert torch.all(ours[0].rnns[0].module.weight_hh_l0 == 0.5)
    assert torch.all(ours[0].rnns[0].weight_hh_l0_raw == 0.5)


def test_tied_decoder_and_hidden_reset_on_batch_change():
    m = get_language_model(**KW).eval()
    assert m[1].decoder.weight.data_ptr() == m[0].encoder.weight.data_ptr()
    m(torch.zeros(1, 1, dtype=torch.long))
    h1 = m[0].hidden[0][0].clone()
    assert h1.abs().sum() > 0
    m(torch.zeros(1, 3, dtype=torch.long))
    assert m[0].bs == 3 and m[0].hidden[0][0].shape[1] == 3


def test_qrnn_unsupported():
    with pytest.raises(NotImplementedError):
        get_language_model(**dict(KW, qrnn=True))


def test_bidirectional_core_matches_reference():
    """bidir=True (reference awd_lstm.py:57,69-70,95): same keys and shapes, same eval forward."""
    kw = dict(KW, bidir=True)
    sd, xs, ys = _ref("awd_lstm_ref_bidir")
    ours = get_language_model(**kw)
    assert set(sd) == set(ours.state_dict())
    for k, v in sd.items():
        assert ours.state_dict()[k].shape == v.shape, k
    ours.load_state_dict(sd)
    ours.eval()
    ours.reset()
    x, a = xs[0], ys[0]
    assert x.shape == (7, 3)
    with torch.no_grad():
        b = ours(x)[0]
    assert a.shape == b.shape and torch.allclose(a, b, atol=1e-5)
    assert ours[0].hidden[0][0].shape == (2, 3, KW["n_hid"] // 2)


def test_bidirectional_checkpoint_refused_by_gpu_packer():
    from hipzap.engine.lm import pack_awd_lstm
    sd = get_language_model(**dict(KW, bidir=True)).state_dict()
    with pytest.raises(ValueError, match="bidirectional"):
        pack_awd_lstm(sd, "cpu")
