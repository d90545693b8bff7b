"""Host layer of the hand-written GEMM family (include/jen1_train.h, jen1_hip.h): what the training graph, the dispatcher ops, the
Encodec modules and the T5 encoder share.

``GemmRuntime``: the library, the compute dtype, ``jen1_train_gemm``'s launch, the split-K accumulator, the launch accounting bench.py
reads, the route switches and the cache of packed compute weights.  ``conv_forward`` / ``conv_dgrad`` / ``conv_wgrad`` run one
convolution / transposed convolution / linear each; WHICH kernel a shape gets is decided by the pure functions ``*_route`` /
``backward_plan`` (integers and flags in, a small tuple out), and every big kernel has one launcher.  No autograd, no fallback.
"""
from __future__ import annotations

import os
import weakref
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import lib as L


def pad8(c: int) -> int:
    return (c + 7) // 8 * 8


class Map:
    """index map of ``jen1_gemm_operand`` (include/jen1_train.h)"""

    def __init__(self, axis: int, L_idx: int, L_src: int, mul: int = 1, tapmul: int = 0, shift: int = 0, div: int = 1, reflect: bool = False,
                 per_batch: bool = False):
        self.axis, self.L, self.Lsrc, self.mul, self.tapmul, self.shift, self.div, self.reflect = axis, L_idx, L_src, mul, tapmul, shift, div, reflect
        self.per_batch = per_batch        # the shift of batch element b comes from jen1_gemm_args.map_shift_b[b] (CausalRows)


_NO_MAP = Map(0, 1, 1)          # rows as they lie

def operand(ptr: int, ld_r: int, ld_k: int, tap_stride: int = 0, zs0: int = 0, zs1: int = 0, zdiv: int = 1,
            m: Optional[Map] = None) -> L.GemmOperand:
    m = m or _NO_MAP
    o = L.GemmOperand()
    o.p, o.zs0, o.zs1, o.ld_r, o.ld_k, o.tap_stride, o.zdiv = ptr, zs0, zs1, ld_r, ld_k, tap_stride, zdiv
    o.map_axis, o.map_L, o.map_Lsrc, o.map_mul, o.map_tapmul, o.map_shift, o.map_div = m.axis, m.L, m.Lsrc, m.mul, m.tapmul, m.shift, m.div
    o.map_reflect, o.reserved = int(m.reflect), int(m.per_batch)
    return o


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def out_rows(like: torch.Tensor, shape, padded: bool) -> torch.Tensor:
    """an output in ``like``'s dtype: zeros when its pitch is padded (the kernels leave the padding lanes alone), else uninitialised"""
    return (torch.zeros if padded else torch.empty)(shape, dtype=like.dtype, device=like.device)


class GemmRuntime:
    """Handle on the library + the per-optimiser-step cache of packed compute weights."""

    def __init__(self, compute_dtype: str = "bf16", device="cuda"):
        self.lib = L.load()                      # raises when the HIP extension is missing
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.Jen1HipError("the training path needs a ROCm GPU (device='cuda'); no CPU path exists in this package")
        assert compute_dtype in ("f32", "bf16")
        self.dt = L.F32 if compute_dtype == "f32" else L.BF16
        self.tdtype = torch.float32 if compute_dtype == "f32" else torch.bfloat16
        self._packed: Dict[tuple, list] = {}          # (id, kind, dtype) -> [weakref, buffer, epoch of last refresh, kind]
        self.epoch = 0
        self._fresh_epoch = -1
        self._acc32: Optional[torch.Tensor] = None        # persistent float32 split-K accumulator, zero at rest
        self.wgrad_plain_rmw = os.environ.get("JEN1_TRAIN_WGRAD_RMW", "1") == "1"
        self._consts: Dict[tuple, torch.Tensor] = {}
        self.stats: Optional[dict] = None        # {"family": [launches, flops, algorithmic bytes]} while a counting pass runs (bench.py)
        self.skinny_gemm = os.environ.get("JEN1_TRAIN_SKINNY", "1") == "1"
        self.fused_repack = os.environ.get("JEN1_TRAIN_FUSED_REPACK", "1") == "1"      # every compute copy in one launch (jen1_repack)
        self.repack_twins = os.environ.get("JEN1_TRAIN_REPACK_TWINS", "1") == "1"      # ... a weight's two copies from one read of it
        self._repack_tab, self._repack_n = None, -1
        self.skinny_max_steps = int(os.environ.get("JEN1_TRAIN_SKINNY_STEPS", "64"))      # K steps per wave
        self.target_wgs = int(os.environ.get("JEN1_TRAIN_TARGET_WGS", "256"))
        self.min_steps = int(os.environ.get("JEN1_TRAIN_MIN_STEPS", "4"))      # K steps (of 32) a split keeps at least
        # weight gradients over many rows (>= big_wgrad_rows) on jen1_big_gemm_tn_conv: 23 us at 24 000 x 128 x (3 x 128) with the bias
        # gradient against 40 on train_gemm's weight-gradient form; the pass 13.58 -> 13.31 ms
        self.big_wgrads = os.environ.get("JEN1_TRAIN_BIG_WGRADS", "1") == "1"
        # forward / data gradient of convolutions over many rows on jen1_big_gemm_conv
        self.big_convs = os.environ.get("JEN1_TRAIN_BIG_CONVS", "1") == "1"
        self.big_conv_rows = int(os.environ.get("JEN1_TRAIN_BIG_CONV_ROWS", "4096"))
        self.big_wgrad_rows = int(os.environ.get("JEN1_TRAIN_BIG_WGRAD_ROWS", "4096"))
        self._banks: Dict[tuple, list] = {}      # (ids of the weights, dtype) -> [weakrefs, weight matrix, weakrefs of the biases, bias vector, epoch]

    def const(self, n: int, v: float) -> torch.Tensor:
        """a cached float32 vector of n copies of v (read-only operands of the glue kernels)"""
        t = self._consts.get((n, v))
        if t is None:
            t = self._consts[(n, v)] = torch.full((n,), float(v), dtype=torch.float32, device=self.device)
        return t

    def stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def invalidate(self) -> None:
        """the parameters changed (optimiser step / load): every packed compute copy is stale"""
        self.epoch += 1

    def dt_of(self, t: torch.Tensor) -> int:
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise L.Jen1HipError(f"unsupported activation dtype {t.dtype}")
        return L.F32 if t.dtype == torch.float32 else L.BF16

    # Conv1d [Co][Ci][k] / ConvTranspose1d [Ci][Co][k] -> [k][Co][Ci]; the data-gradient copies ("D"): rows = input channels, K = output
    # channels contiguous (register-direct GEMM path), [k][Ci][Co]
    _PERMUTE = {"conv": (2, 0, 1), "convT": (2, 1, 0), "convD": (2, 1, 0), "convTD": (2, 0, 1)}

    @staticmethod
    def _layout(w: torch.Tensor, kind: str) -> torch.Tensor:
        d = w.detach()
        if kind in ("linear", "linearD"):
            return (d if kind == "linear" else d.t()).unsqueeze(0)      # [1][Co][Ci] / [1][Ci][Co]
        return d.permute(*GemmRuntime._PERMUTE[kind])

    def packed(self, w: torch.Tensor, kind: str, dtype: torch.dtype) -> torch.Tensor:
        """compute copy [k][C_out][pad8(C_in)] of a Conv1d [Co, Ci, k] / ConvTranspose1d [Ci, Co, k] / Linear [Co, Ci]
        weight.  The buffer is allocated once and refreshed IN PLACE when the parameters moved, so a captured graph
        keeps reading the same address (GraphedLossStep refreshes outside the graph, once per optimiser step)."""
        key = (id(w), kind, dtype)
        hit = self._packed.get(key)
        if hit is not None and hit[0]() is not w:          # id() of a dead parameter can be reused
            hit = None
        if hit is None:
            with torch.no_grad():
                d = self._layout(w, kind)
                k, co, ci = d.shape
                if kind == "linear" and dtype == d.dtype and ci % 8 == 0:
                    hit = [weakref.ref(w), d, -1, kind]    # float32 mode: the parameter itself is the compute copy
                else:
                    hit = [weakref.ref(w), torch.zeros((k, co, pad8(ci)), dtype=dtype, device=w.device), -2, kind]
            self._packed[key] = hit
        if hit[2] != self.epoch and hit[2] != -1:
            self._refresh(hit, w)
        return hit[1]

    def packed_bank(self, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor], dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
        """Compute copies of several Linear weights of one input width as ONE matrix [1][sum C_out][pad8(C_in)] (+ their biases as one
        float32 vector): each weight's copy is a row slice of it, registered like any other packed copy (refreshed by the same
        jen1_repack launch).  The C_out must be multiples of 8 (slices start on 16-byte boundaries in either dtype)."""
        key = (tuple(id(w) for w in weights), dtype)
        hit = self._banks.get(key)
        if hit is not None and any(r() is not w for r, w in zip(hit[0], weights)):
            hit = None
        if hit is None:
            ci = weights[0].shape[1]
            assert all(w.shape[1] == ci and w.shape[0] % 8 == 0 and w.dtype == torch.float32 for w in weights)
            assert all(b.shape[0] == w.shape[0] for w, b in zip(weights, biases))
            total = sum(w.shape[0] for w in weights)
            dev = weights[0].device
            mat = torch.zeros((1, total, pad8(ci)), dtype=dtype, device=dev)
            off = 0
            for w in weights:
                self._packed[(id(w), "linear", dtype)] = [weakref.ref(w), mat[:, off:off + w.shape[0], :], -2, "linear"]
                off += w.shape[0]
            self._repack_tab = None                # (entries may have been replaced: rebuild the table of jen1_repack)
            hit = [[weakref.ref(w) for w in weights], mat, [weakref.ref(b) for b in biases],
                   torch.zeros(total, dtype=torch.float32, device=dev), -2]
            self._banks[key] = hit
        for w in weights:
            self.packed(w, "linear", dtype)        # (refreshes a stale slice; after refresh_all none is)
        self._refresh_bank_bias(hit)
        return hit[1], hit[3]

    def _refresh_bank_bias(self, hit) -> None:
        if hit[4] != self.epoch:
            bs = [r() for r in hit[2]]
            if all(b is not None for b in bs):
                with torch.no_grad():
                    torch.cat([b.detach() for b in bs], out=hit[3])
            hit[4] = self.epoch

    def _refresh(self, hit, w) -> None:
        with torch.no_grad():
            d = self._layout(w, hit[3])
            hit[1][:, :, :d.shape[2]].copy_(d)
        hit[2] = self.epoch

    def refresh_all(self) -> None:
        """bring every packed copy up to date now (outside any graph capture)"""
        if self._fresh_epoch == self.epoch:
            return
        for bank in self._banks.values():
            self._refresh_bank_bias(bank)
        live = [(hit, hit[0]()) for hit in self._packed.values() if hit[2] != -1]
        live = [(hit, w) for hit, w in live if w is not None]
        if self.fused_repack and live:
            # ONE launch for every copy (jen1_repack): the table of (source view, destination) is rebuilt when a copy was added
            if self._repack_tab is None or self._repack_n != len(self._packed):
                self._repack_tab = []              # one table per destination dtype (the time MLPs keep float32 copies in bf16 mode)
                for dt_t, dt_c in ((torch.float32, L.F32), (torch.bfloat16, L.BF16)):
                    ents, t0 = [], 0
                    # a weight's forward copy [k][Co][Ci] and its data-gradient transpose [k][Ci][Co] come from ONE read (dst2)
                    twins = {(id(w), hit[3][:-1]): hit for hit, w in live if hit[1].dtype == dt_t and hit[3].endswith("D")} if self.repack_twins else {}
                    fwd = {(id(w), hit[3]) for hit, w in live if hit[1].dtype == dt_t and not hit[3].endswith("D")}
                    for hit, w in live:
                        if hit[1].dtype != dt_t or (hit[3].endswith("D") and twins and (id(w), hit[3][:-1]) in fwd):
                            continue                   # (a transpose whose forward copy is in this table rides on that entry)
                        d = self._layout(w, hit[3])
                        assert w.dtype == torch.float32
                        e = L.RepackEntry()
                        e.src, e.dst = d.data_ptr(), hit[1].data_ptr()
                        e.d0, e.d1, e.d2, e.ld = d.shape[0], d.shape[1], d.shape[2], hit[1].shape[2]
                        e.s0, e.s1, e.s2 = d.stride(0), d.stride(1), d.stride(2)
                        twin = twins.get((id(w), hit[3]))
                        if twin is not None and twin[0]() is w:
                            assert twin[1].shape[0] == d.shape[0] and twin[1].shape[1] == d.shape[2] and twin[1].shape[2] >= d.shape[1]
                            e.dst2, e.ld2 = twin[1].data_ptr(), twin[1].shape[2]
                        e.tile0 = t0
                        t0 += d.shape[0] * ((d.shape[1] + 31) // 32) * ((d.shape[2] + 31) // 32)
                        ents.append(e)
                    if ents:
                        arr = (L.RepackEntry * len(ents))(*ents)
                        self._repack_tab.append((torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device), len(ents), t0, dt_c))
                self._repack_n = len(self._packed)
            for tab, n, tiles, dt_c in self._repack_tab:
                L.check(self.lib.jen1_repack(tab.data_ptr(), n, tiles, dt_c, self.stream()), "jen1_repack")
            for hit, _ in live:
                hit[2] = self.epoch
        else:
            for hit, w in live:
                if hit[2] != self.epoch:
                    self._refresh(hit, w)
        self._fresh_epoch = self.epoch

    def gemm(self, a: L.GemmOperand, b: L.GemmOperand, c_ptr: int, M: int, N: int, K: int, *, dtype: int, taps: int = 1,
             batches: int = 1, taps_in_z: bool = False, ldc_m: int, ldc_n: int = 1, c_tap_stride: int = 0, c_zs0: int = 0,
             c_zs1: int = 0, c_zdiv: int = 1, bias: Optional[torch.Tensor] = None, splitk: int = 1, atomic: bool = False,
             accumulate: bool = False, c_f32: bool = False, alpha: float = 1.0, rowsum: Optional[torch.Tensor] = None,
             residual: Optional[torch.Tensor] = None, skinny: bool = False, defer: bool = False, pair_with=None,
             shift_b: Optional[torch.Tensor] = None):
        """``defer``: no launch, the filled argument block comes back; ``pair_with`` (such a block): both products in ONE launch
        (jen1_train_gemm_pair: the deferred one first)"""
        g = L.GemmArgs()
        g.a, g.b, g.c, g.bias = a, b, c_ptr, _ptr(bias)
        g.c_zs0, g.c_zs1, g.ldc_m, g.ldc_n, g.c_tap_stride, g.c_zdiv = c_zs0, c_zs1, ldc_m, ldc_n, c_tap_stride, c_zdiv
        g.M, g.N, g.K, g.taps, g.batches = M, N, K, taps, batches
        g.taps_in_z, g.splitk, g.atomic, g.accumulate, g.c_f32, g.dtype = int(taps_in_z), splitk, int(atomic), int(accumulate), int(c_f32), dtype
        g.alpha, g.reserved = alpha, int(skinny)
        g.rowsum, g.residual, g.map_shift_b = _ptr(rowsum), _ptr(residual), _ptr(shift_b)
        if self.stats is not None:
            # executed work of the launch (bench.py's training roofline counts the pass's OWN launch list): 2 M N K per tap and batch;
            # algorithmic bytes = the two operands once + the result (float32 read-modify-write when it accumulates)
            es = 4 if dtype == L.F32 else 2
            by = (M * K * taps + N * K * taps) * batches * es + M * N * batches * (taps if taps_in_z else 1) * ((8 if (atomic or accumulate) else 4) if c_f32 else es)
            self.count("train_gemm", 2.0 * M * N * K * taps * batches, by, launches=0 if pair_with is not None else 1)   # (a pair is one launch)
        if defer:
            return g
        if pair_with is not None:
            L.check(self.lib.jen1_train_gemm_pair(pair_with, g, self.stream()), "jen1_train_gemm_pair")
        else:
            L.check(self.lib.jen1_train_gemm(g, self.stream()), "jen1_train_gemm")
        return None

    def split_accumulator(self, n: int) -> torch.Tensor:
        """the persistent zeroed float32 scratch every split-K forward / data-gradient GEMM of the stream accumulates
        into; ``hand_over`` converts it into the output and zeroes it again in the same launch"""
        if self._acc32 is None or self._acc32.numel() < n:
            assert not torch.cuda.is_current_stream_capturing(), "the split-K accumulator must be sized before graph capture"
            self._acc32 = torch.zeros(max(n, 1 << 23), dtype=torch.float32, device=self.device)
        return self._acc32

    def hand_over(self, acc: torch.Tensor, out: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        tail = (out.numel(), self.dt_of(out), self.stream())
        if residual is not None:
            L.check(self.lib.jen1_convert_clear_add(acc.data_ptr(), out.data_ptr(), residual.data_ptr(), *tail), "jen1_convert_clear_add")
        else:
            L.check(self.lib.jen1_convert_clear(acc.data_ptr(), out.data_ptr(), *tail), "jen1_convert_clear")
        return out

    def count(self, family: str, flops: float, nbytes: float, launches: int = 1) -> None:
        """a launch of ``family`` in the counting pass of bench.py"""
        if self.stats is not None:
            e = self.stats.setdefault(family, [0, 0.0, 0.0])
            e[0] += launches; e[1] += flops; e[2] += nbytes


# =====================================================================================================================
# routes: which kernel a shape gets.  ``sw``: any object with the switch attributes of GemmRuntime (a SimpleNamespace will do)
# =====================================================================================================================
def want_skinny(sw, M: int, N: int, ksteps: int) -> bool:
    """few rows against a big weight: 32 x 16 tiles with the K split inside the workgroup (train_gemm_skinny_kernel) instead of a
    split-K launch + conversion; as long as that gives the chip enough workgroups of a reasonable length"""
    if not sw.skinny_gemm:
        return False
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    wgs = ((M + 31) // 32) * ((N + 15) // 16)
    return tiles < sw.target_wgs // 2 and wgs <= 4096 and ksteps <= 4 * sw.skinny_max_steps


def pick_splitk(sw, M: int, N: int, ksteps: int, z: int = 1) -> int:
    tiles = ((M + 63) // 64) * ((N + 63) // 64) * z
    if tiles >= sw.target_wgs // 2:
        return 1
    # (a few rows against a very long K -- the data gradient of the stacked FiLM projections, 16 x 512 x 55 296: the output is tiny, the
    # atomics cost nothing, and 256 workgroups of 54 serial steps took 82 us)
    wgs = sw.target_wgs * (4 if (M <= 64 and ksteps >= 1024) else 1)
    s = min(max(1, wgs // tiles), max(1, ksteps // sw.min_steps))
    return max(1, min(s, 65535 // max(1, z)))


def _gemm_route(sw, M: int, n_skinny: int, n_split: int, ksteps: int, may_skinny: bool = True, z: int = 1) -> tuple:
    """the forms of jen1_train_gemm: ("skinny",), ("splitk", n) or ("plain",)"""
    if may_skinny and want_skinny(sw, M, n_skinny, ksteps):
        return ("skinny",)
    n = pick_splitk(sw, M, n_split, ksteps, z)
    return ("splitk", n) if n > 1 else ("plain",)


def forward_route(sw, kind: str, rows: int, ci: int, cip: int, co: int, taps: int, dt: int, reflect: bool = False) -> tuple:
    """``rows`` output rows of ``co`` channels from ``taps`` x ``cip`` (= the padded ``ci``) input lanes"""
    if sw.big_convs and dt == L.BF16 and rows >= sw.big_conv_rows and co % 4 == 0:
        if kind in ("conv", "linear") and not reflect and cip % 8 == 0:
            return ("big",)                # jen1_big_gemm_conv, the taps in its row map
        if kind == "convT" and ci % 64 == 0 and cip == ci:
            return ("big_transposed",)     # ... taps reversed, the stride as the divisor of the row map
    return _gemm_route(sw, rows, co, co, taps * ((cip + 31) // 32))


def dgrad_route(sw, kind: str, rows: int, ci_n: int, cip: int, kdim: int, ldy: int, taps: int, dt: int, has_wd: bool, paired: bool) -> tuple:
    """``rows`` input rows of pitch ``cip``, ``ci_n`` of them computed (the rows of ``wd``), reduction over ``kdim`` (``ldy`` with ``wd``)"""
    if sw.big_convs and has_wd and not paired and dt == L.BF16 and ldy % 64 == 0 and ci_n % 4 == 0:
        if kind in ("conv", "linear") and rows >= sw.big_conv_rows:
            return ("big",)                # the conv kernel on dy, taps reversed, pad' = taps - 1 - pad
        if kind == "convT" and rows >= sw.big_conv_rows // 4:
            return ("big_transposed",)     # ConvTranspose1d's data gradient IS a strided convolution of dY
    # (as measured and tuned: skinny is decided from the computed columns ci_n, the split-K factor from the padded pitch cip)
    return _gemm_route(sw, rows, ci_n, cip, taps * ((kdim + 31) // 32), may_skinny=has_wd)


def wgrad_route(sw, kind: str, K: int, co: int, ci: int, ldx: int, ldy: int, taps: int, dt: int, L_in: int, L_out: int, rows_x: int, rows_dy: int,
                reflect: bool, contiguous: bool, deferred: bool) -> tuple:
    """``K`` reduction rows (dy's for Conv1d / Linear, x's for ConvTranspose1d); ``contiguous``: x, dy and the gradient buffer all are"""
    if sw.big_wgrads and not deferred and dt == L.BF16 and contiguous and co % 8 == 0:
        if (kind in ("conv", "linear") and K >= sw.big_wgrad_rows and not reflect and K % L_out == 0 and rows_x * L_out == K * L_in
                and (co % 128 == 0 or ldy >= -(-co // 128) * 128)):
            return ("big",)                # jen1_big_gemm_tn_conv: dy the row operand, the bias gradient as one more MFMA
        if (kind == "convT" and K >= sw.big_wgrad_rows // 4 and ci % 8 == 0 and taps <= 16 and K % L_in == 0 and rows_dy * L_in == K * L_out
                and (ci % 128 == 0 or ldx >= -(-ci // 128) * 128)):
            return ("big_transposed",)     # ... the input as its row operand and dY as the shifted one
    M, N = (ci, co) if kind == "convT" else (co, ci)
    return _gemm_route(sw, M, N, N, (K + 31) // 32, may_skinny=False, z=taps)


def backward_plan(sw, kind: str, rows: int, ci: int, dt: int, need_dx: bool) -> tuple:
    """a layer's two gradients: ("pair",) one launch for both; ("queue",) the weight gradient on its own, through the weight-gradient
    queue (many-row layers: both products fill the chip, a pair would last their sum)"""
    many_rows = ((rows + 63) // 64) * ((ci + 63) // 64) >= sw.target_wgs or (
        sw.big_wgrads and sw.big_wgrad_unpair and rows >= sw.big_wgrad_rows and kind in ("conv", "linear") and dt == L.BF16)
    return ("pair",) if (need_dx and sw.pair_grads and not many_rows) else ("queue",)


# launchers: the only places that pass these argument lists positionally (keyword names: include/jen1_hip.h)
def launch_big_conv(rt: GemmRuntime, *, x, w, bias, residual, y, B, T_in, T_out, ci, co, taps, stride, pad, tap_rev, ld_x, ld_w, w_tap_stride, ld_y,
                    shift_b, div, flops: float, nbytes: float) -> None:
    L.check(rt.lib.jen1_big_gemm_conv(x.data_ptr(), w.data_ptr(), _ptr(bias), _ptr(residual), y.data_ptr(), B, T_in, T_out, ci, co, taps, stride, pad,
                                      tap_rev, ld_x, ld_w, w_tap_stride, ld_y, _ptr(shift_b), div, rt.stream()), "jen1_big_gemm_conv")
    rt.count("big_gemm", flops, nbytes)


def launch_big_tn_conv(rt: GemmRuntime, *, dy, x, gw, gb, B, T_out, T_in, co, ci, taps, stride, pad, ld_dy, ld_x, shift_b, flops: float,
                       nbytes: float) -> None:
    L.check(rt.lib.jen1_big_gemm_tn_conv(dy.data_ptr(), x.data_ptr(), gw.data_ptr(), _ptr(gb), B, T_out, T_in, co, ci, taps, stride, pad, ld_dy, ld_x,
                                         1.0, _ptr(shift_b), rt.stream()), "jen1_big_gemm_tn_conv")
    rt.count("big_gemm", flops, nbytes)


def big_gemm(rt: GemmRuntime, a2d: torch.Tensor, b2d: torch.Tensor, out: torch.Tensor, K: int, bias: Optional[torch.Tensor] = None) -> None:
    """out[M][N] = a2d[M][:K] @ b2d[N][:K]^T (+ bias[N], float32) on jen1_big_gemm (one column group)"""
    g = L.BGemmArgs()
    g.a, g.b, g.c, g.ldc = a2d.data_ptr(), b2d.data_ptr(), out.data_ptr(), out.stride(0)      # (one inline group: nothing to copy while capturing)
    g.bias = _ptr(bias)
    g.M, g.Ntot, g.K, g.lda, g.ldb, g.n_groups = a2d.shape[0], b2d.shape[0], K, a2d.stride(0), b2d.stride(0), 1
    g.dtype, g.alpha = rt.dt_of(a2d), 1.0
    rt.count("big_gemm", 2.0 * a2d.shape[0] * b2d.shape[0] * K, (a2d.shape[0] * K + b2d.shape[0] * K + a2d.shape[0] * b2d.shape[0]) * a2d.element_size())
    L.check(rt.lib.jen1_big_gemm(g, rt.stream()), "jen1_big_gemm")


def bias_grad(rt: GemmRuntime, dy: torch.Tensor, gb: torch.Tensor, co: int) -> None:
    """gb[co] (float32) += the column sums of dy: the bias gradient where no GEMM carries it"""
    ldy = dy.shape[-1]
    L.check(rt.lib.jen1_colsum(dy.data_ptr(), gb.data_ptr(), dy.numel() // ldy, co, ldy, rt.dt_of(dy), rt.stream()), "jen1_colsum")


def compute_copy(w: torch.Tensor, kind: str, dtype: torch.dtype) -> torch.Tensor:
    """a one-off compute copy [k][rows][pad8(columns)] of a weight (``GemmRuntime.packed`` without the cache)"""
    d = GemmRuntime._layout(w, kind)
    out = torch.zeros((d.shape[0], d.shape[1], pad8(d.shape[2])), dtype=dtype, device=w.device)
    out[:, :, :d.shape[2]] = d
    return out


# =====================================================================================================================
# convolution family: _Conv1d (blocks.py:34-53), nn.Conv1d / nn.ConvTranspose1d of Upsample1d (blocks.py:69-95), nn.Linear
# =====================================================================================================================
class ConvGeom:
    """static description of one convolution call"""

    def __init__(self, kind: str, taps: int, stride: int, pad: int, L_in: int, L_out: int, ci: int, co: int, reflect: bool = False,
                 pad_b: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        self.kind, self.taps, self.stride, self.pad, self.L_in, self.L_out, self.ci, self.co = kind, taps, stride, pad, L_in, L_out, ci, co
        self.reflect = reflect        # forward only: F.pad(mode="reflect") instead of zeros (SEANet convolutions)
        # (-pad, +pad) per batch element as int32 tensors: a pass that mixes causal and non-causal clips ("conv" kind only)
        self.pad_b = pad_b
        self.fwd_shift_b, self.bwd_shift_b = pad_b if pad_b is not None else (None, None)
        self.big_pad = 0 if pad_b is not None else pad        # the big kernels take a per-batch padding in shift_b alone
        assert pad_b is None or kind == "conv"
        assert kind != "linear" or (taps, stride, pad) == (1, 1, 0)

    def fwd_map(self, axis: int) -> Optional[Map]:
        """activation index (b, t_out) [+ tap] -> input row"""
        if self.kind == "linear":
            return None
        if self.kind == "conv":
            return Map(axis, self.L_out, self.L_in, mul=self.stride, tapmul=1, shift=-self.pad, reflect=self.reflect,
                       per_batch=self.pad_b is not None)
        return Map(axis, self.L_out, self.L_in, mul=1, tapmul=-1, shift=self.pad, div=self.stride)

    def bwd_map(self, axis: int) -> Optional[Map]:
        """activation index (b, t_in) [+ tap] -> output row"""
        if self.kind == "linear":
            return None
        if self.kind == "conv":
            return Map(axis, self.L_in, self.L_out, mul=1, tapmul=-1, shift=self.pad, div=self.stride, per_batch=self.pad_b is not None)
        return Map(axis, self.L_in, self.L_out, mul=self.stride, tapmul=1, shift=-self.pad)


def _train_gemm_rows(rt: GemmRuntime, route: tuple, a, b, like: torch.Tensor, shape, N: int, K: int, residual, **kw) -> torch.Tensor:
    """[B, L, ld] (``shape``) = a b^T over N columns (+ ``residual``) on jen1_train_gemm, in the form ``route`` names"""
    M, ld = shape[0] * shape[1], shape[2]
    if route[0] == "splitk":
        acc = rt.split_accumulator(M * ld)
        rt.gemm(a, b, acc.data_ptr(), M, N, K, ldc_m=ld, splitk=route[1], atomic=True, c_f32=True, **kw)
        return rt.hand_over(acc, out_rows(like, shape, False), residual)
    if residual is not None and ld != N:
        y = residual.clone()                   # (padding columns: keep the residual's)
        rt.gemm(a, b, y.data_ptr(), M, N, K, ldc_m=ld, accumulate=True, skinny=route[0] == "skinny", **kw)
        return y
    y = out_rows(like, shape, ld != N)
    rt.gemm(a, b, y.data_ptr(), M, N, K, ldc_m=ld, residual=residual, skinny=route[0] == "skinny", **kw)
    return y


def conv_forward(rt: GemmRuntime, x: torch.Tensor, wp: torch.Tensor, bias: Optional[torch.Tensor], g: ConvGeom,
                 residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x: [..rows.., ldx] channel-last with ldx == wp.shape[2]; returns [B, L_out, pad8(co)] (+ ``residual`` of that shape, added in
    the epilogue of the GEMM or of the split-K hand-over)"""
    dt = rt.dt_of(x)
    ldx = x.shape[-1]
    k, co, cip = wp.shape
    assert ldx == cip and x.is_contiguous() and k == g.taps and co == g.co, (x.shape, wp.shape, g.__dict__)
    rows_in = x.numel() // ldx
    B = rows_in // g.L_in
    M = B * g.L_out
    ldy = pad8(co)
    shape = (B, g.L_out, ldy)
    assert residual is None or (residual.is_contiguous() and residual.numel() == M * ldy and residual.dtype == x.dtype), (residual.shape, shape)
    route = forward_route(rt, g.kind, M, g.ci, cip, co, k, dt, g.reflect)
    if route[0] in ("big", "big_transposed"):
        # the 128 x 128 matrix-core kernel (10 us at 24 000 x 128 x (3 x 128) against 25 on the register-direct form).  ConvTranspose1d: output
        # position t reads input (t + padding - tap) / stride where that is whole (the other taps' rows arrive as zeros: wasted MFMA steps only)
        y = out_rows(x, shape, ldy != co)
        nb, t_in, t_out = (B, g.L_in, g.L_out) if g.kind != "linear" else (M, 1, 1)      # (a linear: one position per row)
        form = (dict(ci=cip, stride=g.stride, pad=g.big_pad, tap_rev=0, shift_b=g.fwd_shift_b, div=1, flops=2.0 * M * co * cip * k) if route[0] == "big" else
                dict(ci=g.ci, stride=1, pad=k - 1 - g.pad, tap_rev=1, shift_b=None, div=g.stride, flops=2.0 * M * co * cip * k / g.stride))
        launch_big_conv(rt, x=x, w=wp, bias=bias, residual=residual, y=y, B=nb, T_in=t_in, T_out=t_out, co=co, taps=k, ld_x=ldx, ld_w=cip,
                        w_tap_stride=co * cip, ld_y=ldy, nbytes=2.0 * (rows_in * ldx + k * co * cip + M * ldy), **form)
        return y
    a = operand(x.data_ptr(), ldx, 1, m=g.fwd_map(1))
    b = operand(wp.data_ptr(), cip, 1, tap_stride=co * cip)
    return _train_gemm_rows(rt, route, a, b, x, shape, co, cip, residual, dtype=dt, taps=k, bias=bias, shift_b=g.fwd_shift_b)


def conv_dgrad(rt: GemmRuntime, dy: torch.Tensor, wp: torch.Tensor, g: ConvGeom, wd: Optional[torch.Tensor] = None, pair_with=None,
               residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``wd``: the data-gradient copy [k][Ci][pad8(Co)] of the weight (both GEMM operands K-contiguous: the register-direct
    path of jen1_train_gemm); without it the forward copy ``wp`` is read transposed through LDS.  ``pair_with``: the deferred
    weight-gradient product of the same layer, launched together with this one.  ``residual`` (dx's shape): added in the epilogue
    (the gradient that reached the layer's input along a branch around it: ConvFn's ``fork``)"""
    dt = rt.dt_of(dy)
    ldy = dy.shape[-1]
    k, co, cip = wp.shape
    assert dy.is_contiguous() and ldy == pad8(co)
    B = dy.numel() // ldy // g.L_out
    M = B * g.L_in
    shape = (B, g.L_in, cip)
    assert wd is None or (wd.shape[0] == k and wd.shape[2] == ldy)
    cip_n, kdim = (wd.shape[1], ldy) if wd is not None else (cip, co)       # (with wd, K runs over the padded (zero) output channels too)
    route = dgrad_route(rt, g.kind, M, cip_n, cip, kdim, ldy, k, dt, wd is not None, pair_with is not None)
    if route[0] in ("big", "big_transposed"):
        # (a strided convolution's data gradient: the stride as the divisor of the row map; ConvTranspose1d's: row t_in stride + tap - padding)
        dx = out_rows(dy, shape, cip_n != cip)
        nb, t_in, t_out = (B, g.L_out, g.L_in) if g.kind != "linear" else (M, 1, 1)
        form = (dict(stride=1, pad=(k - 1) if g.pad_b is not None else (k - 1 - g.pad), tap_rev=1, shift_b=g.bwd_shift_b, div=g.stride) if route[0] == "big" else
                dict(stride=g.stride, pad=g.pad, tap_rev=0, shift_b=None, div=1))
        launch_big_conv(rt, x=dy, w=wd, bias=None, residual=residual, y=dx, B=nb, T_in=t_in, T_out=t_out, ci=ldy, co=cip_n, taps=k, ld_x=ldy, ld_w=ldy,
                        w_tap_stride=cip_n * ldy, ld_y=cip, flops=2.0 * M * cip_n * ldy * k, nbytes=2.0 * (B * g.L_out * ldy + k * cip_n * ldy + M * cip), **form)
        return dx
    a = operand(dy.data_ptr(), ldy, 1, m=g.bwd_map(1))
    b = operand(wd.data_ptr(), ldy, 1, tap_stride=cip_n * ldy) if wd is not None else operand(wp.data_ptr(), 1, cip, tap_stride=co * cip)
    return _train_gemm_rows(rt, route, a, b, dy, shape, cip_n, kdim, residual, dtype=dt, taps=k, pair_with=pair_with, shift_b=g.bwd_shift_b)


def conv_wgrad(rt: GemmRuntime, x: torch.Tensor, dy: torch.Tensor, gw: torch.Tensor, g: ConvGeom, gb: Optional[torch.Tensor] = None,
               defer: bool = False):
    """gw (float32, reference layout) += the weight gradient.  ``gb`` (bias gradient) is accumulated by the same launch
    when dy is the row operand (Conv1d / Linear); returns whether it was -- with ``defer`` (whether, the argument block of the
    launch that has NOT been issued)."""
    dt = rt.dt_of(x)
    ldx, ldy = x.shape[-1], dy.shape[-1]
    rows_x, rows_dy = x.numel() // ldx, dy.numel() // ldy
    if not dy.is_contiguous():                 # a column slice of a wider matrix (FilmBankFn): rows dy.stride(0) apart
        assert dy.dim() == 2 and dy.stride(1) == 1 and g.kind == "linear"
        ldy = dy.stride(0)
    k = g.taps
    K = rows_x if g.kind == "convT" else rows_dy
    route = wgrad_route(rt, g.kind, K, g.co, g.ci, ldx, ldy, k, dt, g.L_in, g.L_out, rows_x, rows_dy, g.reflect,
                        x.is_contiguous() and dy.is_contiguous() and gw.is_contiguous(), defer)
    if route[0] == "big":
        launch_big_tn_conv(rt, dy=dy, x=x, gw=gw, gb=gb, B=K // g.L_out, T_out=g.L_out, T_in=g.L_in, co=g.co, ci=g.ci, taps=k, stride=g.stride, pad=g.big_pad,
                           ld_dy=ldy, ld_x=ldx, shift_b=g.fwd_shift_b, flops=2.0 * K * g.co * g.ci * k, nbytes=2.0 * K * (g.co + g.ci) + 8.0 * g.co * g.ci * k)
        return gb is not None
    if route[0] == "big_transposed":
        # dW[ci][co][tap] = sum x[b, t][ci] dy[b, t stride + tap - padding][co] (82 us on train_gemm's weight-gradient form at
        # 6 000 x 128 x (8 x 128)); this form never fuses the bias gradient
        launch_big_tn_conv(rt, dy=x, x=dy, gw=gw, gb=None, B=K // g.L_in, T_out=g.L_in, T_in=g.L_out, co=g.ci, ci=g.co, taps=k, stride=g.stride, pad=g.pad,
                           ld_dy=ldx, ld_x=ldy, shift_b=None, flops=2.0 * K * g.co * g.ci * k, nbytes=2.0 * (K * g.ci + rows_dy * g.co) + 8.0 * g.co * g.ci * k)
        return False
    if g.kind == "convT":
        # W[ci][co][k]: rows m = ci from x (K = (b, t_in)), rows n = co from dy at the mapped row
        a, b, M, N = operand(x.data_ptr(), 1, ldx), operand(dy.data_ptr(), 1, ldy, m=g.bwd_map(2)), g.ci, g.co
    else:
        # W[co][ci][k]: rows m = co from dy (K = (b, t_out)), rows n = ci from x at the mapped row
        a, b, M, N = operand(dy.data_ptr(), 1, ldy), operand(x.data_ptr(), 1, ldx, m=g.fwd_map(2)), g.co, g.ci
    sk = route[1] if route[0] == "splitk" else 1
    fused_bias = gb is not None and g.kind != "convT"
    # one K slice: every (tap, tile) of the gradient belongs to exactly one workgroup of this launch and launches are
    # stream-ordered, so a plain read-modify-write accumulates; float atomics only when the K range is split
    na = sk == 1 and rt.wgrad_plain_rmw
    blk = rt.gemm(a, b, gw.data_ptr(), M, N, K, dtype=dt, taps=k, taps_in_z=True, ldc_m=N * k, ldc_n=k, c_tap_stride=1,
                  splitk=sk, atomic=not na, accumulate=na, c_f32=True, rowsum=gb if fused_bias else None, defer=defer,
                  shift_b=g.fwd_shift_b if g.kind == "conv" else None)
    return (fused_bias, blk) if defer else fused_bias
