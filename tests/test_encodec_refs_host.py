"""CPU: the float64 references of tests/encodec_common.py, pinned against torch.nn.LSTM (float64) and the numpy oracle, so that the GPU
kernel tests (tests/test_gpu_encodec_kernels.py) compare with something that is itself known to be right."""
import numpy as np
import torch

from encodec_common import bf16_round, lstm_inputs, lstm_layer_emul, lstm_layer_ref, rvq_decode_ref
from helpers import rel_err


def test_lstm_layer_ref_matches_torch_lstm_float64():
    H, B, T = 256, 3, 17
    g = torch.Generator().manual_seed(11)
    lstm = torch.nn.LSTM(H, H, num_layers=1, batch_first=True).double()
    with torch.no_grad():
        for p in lstm.parameters():
            p.copy_((torch.rand(p.shape, generator=g, dtype=torch.float64) * 2 - 1) * H ** -0.5)
        x = torch.randn((B, T, H), generator=g, dtype=torch.float64)
        want, _ = lstm(x)
        gin = x @ lstm.weight_ih_l0.T + lstm.bias_ih_l0 + lstm.bias_hh_l0          # weight_ih and both biases folded into gin
    got = lstm_layer_ref(gin.numpy(), lstm.weight_hh_l0.detach().numpy())
    assert got.dtype == np.float64 and got.shape == (B, T, H)
    assert float(np.abs(got - want.numpy()).max()) <= 1e-12
    skip = torch.randn((B, T, H), generator=g, dtype=torch.float64).numpy()
    assert np.array_equal(lstm_layer_ref(gin.numpy(), lstm.weight_hh_l0.detach().numpy(), skip), got + skip)


def test_lstm_layer_ref_twice_matches_oracle_slstm():
    """two layers, the skip on the second: the oracle's fused float32 SLSTM"""
    from oracle import encodec_oracle as EO
    H, B, T = 64, 2, 23
    rng = np.random.default_rng(5)
    p = {}
    for l in range(2):
        p[f"m.lstm.weight_ih_l{l}"] = (rng.uniform(-1, 1, (4 * H, H)) * H ** -0.5).astype(np.float32)
        p[f"m.lstm.weight_hh_l{l}"] = (rng.uniform(-1, 1, (4 * H, H)) * H ** -0.5).astype(np.float32)
        p[f"m.lstm.bias_ih_l{l}"] = rng.uniform(-0.1, 0.1, 4 * H).astype(np.float32)
        p[f"m.lstm.bias_hh_l{l}"] = rng.uniform(-0.1, 0.1, 4 * H).astype(np.float32)
    x = rng.standard_normal((B, H, T)).astype(np.float32)
    want = EO.slstm(x, p, "m", 2)                                  # [B, H, T]
    rows = x.transpose(0, 2, 1).astype(np.float64)                 # [B, T, H]
    h = rows
    for l in range(2):
        gin = h @ p[f"m.lstm.weight_ih_l{l}"].astype(np.float64).T + (p[f"m.lstm.bias_ih_l{l}"].astype(np.float64) + p[f"m.lstm.bias_hh_l{l}"])
        h = lstm_layer_ref(gin, p[f"m.lstm.weight_hh_l{l}"], rows if l == 1 else None)
    assert rel_err(want, h.transpose(0, 2, 1)) <= 1e-5


def test_lstm_emulations_sit_where_the_gates_assume():
    """the float32 restatement is within a few 1e-7 of the float64 layer and the bf16 hi + lo form within a few 1e-6: the GPU gates are
    8x these figures, computed per case"""
    gin, whh, skip = lstm_inputs(3, 33, 256, 7)
    ref = lstm_layer_ref(gin, whh, skip)
    e32 = float(np.abs(lstm_layer_emul(gin, whh, skip) - ref).max())
    whh16 = bf16_round(whh)
    ehl = float(np.abs(lstm_layer_emul(gin, whh16, skip, split_h=True) - lstm_layer_ref(gin, whh16, skip)).max())
    assert 0 < e32 < 1e-6 and 0 < ehl < 4e-6, (e32, ehl)
    # rounding the weights to bf16 moves the layer by far more than either: a kernel that used the wrong precision would be seen
    assert float(np.abs(lstm_layer_ref(gin, whh16, skip) - ref).max()) > 50 * e32


def test_bf16_round_is_round_to_nearest_even():
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 3 * 2.0 ** -8, -3.0e4, 0.0], dtype=np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, -29952.0, 0.0], dtype=np.float32)
    assert np.array_equal(bf16_round(a), want)


def test_rvq_decode_ref_matches_oracle_and_clamps():
    from oracle import encodec_oracle as EO
    rng = np.random.default_rng(3)
    n_q, B, T, bins, D = 4, 2, 37, 16, 64
    tables = rng.standard_normal((n_q, bins, D)).astype(np.float32)
    codes = rng.integers(0, bins, (n_q, B, T))
    codes[0, 0, 0], codes[1, 1, 5] = 3, 2
    got = rvq_decode_ref(codes, tables)
    assert got.dtype == np.float64 and got.shape == (B, D, T)
    assert rel_err(EO.rvq_decode(codes, tables), got) <= 1e-6
    assert np.all(rvq_decode_ref(codes, tables, magnitude=True) >= np.abs(got))
    # fewer codebooks than tables: the first ones
    assert np.array_equal(rvq_decode_ref(codes[:1], tables), tables[0].astype(np.float64)[codes[0]].transpose(0, 2, 1))
    bad = codes.copy()
    bad[0, 0, 0], bad[1, 1, 5] = -1, bins
    fixed = codes.copy()
    fixed[0, 0, 0], fixed[1, 1, 5] = 0, bins - 1
    assert np.array_equal(rvq_decode_ref(bad, tables), rvq_decode_ref(fixed, tables))
    assert not np.array_equal(rvq_decode_ref(bad, tables), got)
