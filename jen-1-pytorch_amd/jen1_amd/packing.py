"""Host-side weight packing into the MFMA fragment order jen1_conv_gemm streams.

Packed layout (DESIGN.md "weights in HBM"):  [tap][c/32][m/16][lane 0..63][8]
with lane = g*16 + i, element j  <->  W[tap][m = 16*mt + i][c = 32*kc + 8*g + j].
One wave-instruction therefore reads one contiguous 1 KiB (bf16) / 2 KiB (f32)
block.  The M tile is the fastest block index on purpose: the workgroups of a launch own
different M tiles and walk K in lockstep, so at any instant their loads form one contiguous
span that spreads over all HBM channels (with M-tile-major blocks they sat 32 KiB apart and
camped on a few channels).

All functions take the reference's parameter tensors (reference ``state_dict``
layouts) and return device tensors in the compute dtype.
"""
from __future__ import annotations

import torch


def _ceil_to(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def pack_gemm_weight(w_tmk: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """w_tmk: [taps][M][K] float32 (already in GEMM form) -> packed [taps][Kp/32][M/16][64][8].
    M must be a multiple of 16; K is zero-padded to a multiple of 32."""
    taps, M, K = w_tmk.shape
    assert M % 16 == 0, M
    Kp = _ceil_to(K, 32)
    if Kp != K:
        w_tmk = torch.nn.functional.pad(w_tmk, (0, Kp - K))
    w = w_tmk.reshape(taps, M // 16, 16, Kp // 32, 4, 8)          # [tap, mt, i, kc, g, j]
    w = w.permute(0, 3, 1, 4, 2, 5).contiguous()                   # [tap, kc, mt, g, i, j]
    return w.reshape(taps, Kp // 32, M // 16, 64, 8).to(dtype).contiguous()


def conv_weight_to_gemm(w: torch.Tensor) -> torch.Tensor:
    """nn.Conv1d weight [C_out][C_in][k] -> [k][C_out][C_in] (reference blocks.py:42)."""
    return w.permute(2, 0, 1).contiguous()


def convT_weight_to_gemm(w: torch.Tensor, f: int) -> torch.Tensor:
    """nn.ConvTranspose1d weight [C_in][C_out][2f] (reference blocks.py:88-95) as a 2-tap
    sub-pixel GEMM: out[q*f + r - p] = x[q] . W[:, :, r] + x[q-1] . W[:, :, r+f].
    Returns [2][f*C_out][C_in] with tap 0 <-> x[q-1], tap 1 <-> x[q]; row m = r*C_out + co."""
    ci, co, k = w.shape
    assert k == 2 * f
    w_r = w.permute(2, 1, 0)                       # [j][co][ci]
    tap1 = w_r[:f].reshape(f * co, ci)             # j = r       <-> x[q]
    tap0 = w_r[f:].reshape(f * co, ci)             # j = r + f   <-> x[q-1]
    return torch.stack([tap0, tap1], dim=0).contiguous()


def fold_layernorm(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor):
    """Linear(LayerNorm(x)) = (W diag(gamma)) xhat + W beta  (reference blocks.py:427-429):
    returns (W', b') so the kernel's LN prologue only standardises."""
    return w * gamma[None, :], w @ beta


def pqkv_matrix(w_proj: torch.Tensor, b_proj: torch.Tensor, w_qkv: torch.Tensor):
    """The transformer's input 1x1 conv and the LayerNorm-folded q / k / v projection that reads its output as ONE dual-range
    map over xh = GN(x):  [x1 | qkv_raw] = [P ; Wqkv' P] xh + [p_b ; Wqkv' p_b]  (reference blocks.py:530-531, :427-429).  The
    LayerNorm finish rstd (raw - mean u) + b is the consumer's.  w_qkv: ``fold_layernorm`` rows [3 mid][C].  Returns
    (W [C + 3 mid][C], bias [C + 3 mid]) in float64."""
    P, pb, wqkv = (w_proj[:, :, 0] if w_proj.dim() == 3 else w_proj).double(), b_proj.double(), w_qkv.double()
    return torch.cat([P, wqkv @ P], 0), torch.cat([pb, wqkv @ pb])


def o1q2_matrix(w_o: torch.Tensor, b_o: torch.Tensor, w_q2: torch.Tensor):
    """Self-attention's output projection and the LayerNorm-folded cross-attention query over the K concat [a1 | x1]:
    [x2 | q2_raw] = [W_o | 0 ; Wq2' W_o | Wq2'] [a1 | x1] + [b_o ; Wq2' b_o]  (+ x1 on the x2 rows: the residual operand of the
    launch).  w_o: [C][mid], w_q2: ``fold_layernorm`` rows [mid][C].  Returns (W [C + mid][mid + C], bias [C + mid]) in float64."""
    wo, bo, wq2 = w_o.double(), b_o.double(), w_q2.double()
    top = torch.cat([wo, torch.zeros(wo.shape[0], wq2.shape[1], dtype=torch.float64, device=wo.device)], 1)
    bot = torch.cat([wq2 @ wo, wq2], 1)
    return torch.cat([top, bot], 0), torch.cat([bo, wq2 @ bo])


def s1q2_matrix(w_o: torch.Tensor, w_v: torch.Tensor, w_q2: torch.Tensor):
    """ONE position: softmax over a single key is 1, so self-attention is to_out(to_v(norm_context(x1))) (reference
    blocks.py:355-380, :427-437) and the whole sub-block is
    [x2 | q2_raw] = [W_o W_v | 0 ; Wq2' W_o W_v | Wq2'] [LN_ctx(x1) | x1] + [b_o ; Wq2' b_o]  (+ x1 on the x2 rows), with the
    bias of ``o1q2_matrix``.  w_v: the v rows of to_kv [mid][C], NOT folded (the launch's one-group GroupNorm prologue applies gamma /
    beta of norm_context).  Returns W [C + mid][C + C] in float64."""
    wo, wq2 = w_o.double(), w_q2.double()
    wc = wo @ w_v.double()
    top = torch.cat([wc, torch.zeros(wc.shape[0], wq2.shape[1], dtype=torch.float64, device=wc.device)], 1)
    bot = torch.cat([wq2 @ wc, wq2], 1)
    return torch.cat([top, bot], 0)


def o2f1_matrix(w_o: torch.Tensor, b_o: torch.Tensor, w_1: torch.Tensor, b_1: torch.Tensor):
    """Cross-attention's output projection and the first FeedForward layer over the K concat [a | x2]:  x3 = x2 + W_o a + b_o  (rows
    < C, K = a only, + x2 as the residual operand) and  f = gelu(W_1 x3 + b_1) = gelu((W_1 W_o) a + W_1 x2 + W_1 b_o + b_1)
    (reference blocks.py:485-488, :440-446).  Returns (W [C + F][mid + C], bias [C + F]) in float64."""
    wo, bo, w1 = w_o.double(), b_o.double(), w_1.double()
    top = torch.cat([wo, torch.zeros(wo.shape[0], w1.shape[1], dtype=torch.float64, device=wo.device)], 1)
    bot = torch.cat([w1 @ wo, w1], 1)
    return torch.cat([top, bot], 0), torch.cat([bo, b_1.double() + w1 @ bo])


def ff_out_matrix(w_proj: torch.Tensor, b_proj: torch.Tensor, w_ff2: torch.Tensor, b_ff2: torch.Tensor):
    """The transformer's tail  y = P (x + W_ff2 f + b_ff2) + b_P  (reference blocks.py:446, :488, :536) as ONE linear map over
    the K concat [x | f]: returns (Wm = [P | P W_ff2]  [C][C + F],  b_m = b_P + P b_ff2) in float64.
    w_proj: the 1x1 conv weight [C][C][1] or [C][C]."""
    P = (w_proj[:, :, 0] if w_proj.dim() == 3 else w_proj).double()
    return torch.cat([P, P @ w_ff2.double()], 1), b_proj.double() + P @ b_ff2.double()


def fold_linear_into_upsample(w_up: torch.Tensor, b_up: torch.Tensor, f: int, wm: torch.Tensor, b_m: torch.Tensor):
    """ConvTranspose1d(y) with y = Wm z + b_m (a 1x1 conv over the K concat z) as ONE 2-tap sub-pixel GEMM over z.

    With U[k] the two packed taps of the transposed conv (``convT_weight_to_gemm``: tap 0 <-> y[q-1], tap 1 <-> y[q]) GEMM
    column q in [0, L] is  U[0] y[q-1] + U[1] y[q] + b_up, and y does not exist outside [0, L): there the staged halo rows of z
    are zero, so the matrix part  Wf[k] = U[k] Wm  needs no edge treatment -- but b_m must not be counted for a tap that falls
    outside the sample.  Returns, in float64,
        Wf      [2][f * C_out][K]    the folded taps,
        b_mid   [f * C_out]          bias of an interior column:  b_up + (U[0] + U[1]) b_m,
        b_first [f * C_out]          bias of column q = 0:        b_up + U[1] b_m,
        b_last  [f * C_out]          bias of column q = L:        b_up + U[0] b_m
    (row m = r * C_out + co as in ``convT_weight_to_gemm``; the biases are per GEMM row because U differs per phase r)."""
    U = convT_weight_to_gemm(w_up.double(), f)            # [2][f * C_out][C]
    wm, b_m = wm.double(), b_m.double()
    bu = b_up.double().repeat(f)
    u0b, u1b = U[0] @ b_m, U[1] @ b_m
    return torch.stack([U[0] @ wm, U[1] @ wm], 0), bu + u0b + u1b, bu + u1b, bu + u0b
