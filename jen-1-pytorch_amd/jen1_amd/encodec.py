"""Encodec 48 kHz pieces either side of the sampler, on the HIP kernels.

What the reference calls on ``EncodecModel.encodec_model_48khz()`` (third-party ``encodec==0.1.1``, requirements.txt:5,
not vendored, weights not available offline):
  * ``audio_encoder.quantizer.decode(codes)``  (generation.py:145-150): codes -> the 128-channel latents the denoiser
    works on  ->  ``ResidualVectorQuantizerHIP.decode`` (jen1_rvq_decode);
  * ``audio_encoder.decoder(sample_embs)``     (generation.py:130): latents ``[B, 128, T]`` -> stereo audio
    ``[B, 2, 320 T]`` through the SEANet decoder  ->  ``SEANetDecoderHIP``.
  * ``audio_encoder.encode(audio)``            (generation.py:146; dataloader.py:106-114): 1 s segments, RMS normalisation,
    SEANet encoder, nearest-codebook search  ->  ``EncodecHIP.encode`` (``SEANetEncoderHIP``,
    ``ResidualVectorQuantizerHIP.encode``).

The decoder restates encodec 0.1.1 ``modules/seanet.py::SEANetDecoder`` with the 48 kHz settings (dimension 128,
n_filters 32, ratios [8, 5, 4, 2], kernel 7, last kernel 7, residual kernel 3, 1 residual layer, compress 2, 2 LSTM
layers, ELU, non-causal, reflect padding, norm "time_group_norm", true skip off): every SConv1d / SConvTranspose1d is
convolution -> GroupNorm(1 group) [-> trim for the transposed ones, AFTER the norm], as in ``modules/conv.py``.
Convolutions run on jen1_train_gemm (the reflect padding is an index map, no padded copy), GroupNorm / ELU on the
train_ops kernels, the LSTM on jen1_lstm_layer.  Parameters are taken under the key names of the Hugging Face port
(``transformers.EncodecModel``: ``layers.N.conv.weight`` ...), which is the implementation of that architecture available offline:
PARITY IS PINNED AGAINST THAT PORT WITH SYNTHETIC WEIGHTS (tests/golden/encodec.npz); the real checkpoint and the
``encodec`` package itself are not available here, so parity against them is unpinned.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Sequence

import torch

from . import lib as L
from .gemm_host import ConvGeom, GemmRuntime, conv_forward, operand, pad8

HOP_48K = 320


class ResidualVectorQuantizerHIP:
    """``quantizer.decode`` (encodec quantization/vq.py ResidualVectorQuantizer.decode -> core_vq decode): the sum over
    the n_q codebooks of the looked-up vectors.  ``tables``: float32 ``[n_q, bins, 128]`` (``layers.q.codebook.embed``)."""

    def __init__(self, tables: torch.Tensor, device="cuda"):
        self.lib = L.load()
        self.tables = tables.to(device, torch.float32).contiguous()
        self.device = torch.device(device)
        self._rt = None
        self.e_sq = (self.tables ** 2).sum(-1).contiguous()                    # [n_q][bins]: |e|^2 of the search score 2 r.e - |e|^2

    @classmethod
    def from_state_dict(cls, sd: Dict[str, torch.Tensor], device="cuda") -> "ResidualVectorQuantizerHIP":
        n = 0
        while f"layers.{n}.codebook.embed" in sd:
            n += 1
        assert n > 0, "no layers.N.codebook.embed entries"
        return cls(torch.stack([sd[f"layers.{q}.codebook.embed"] for q in range(n)]), device)

    @torch.no_grad()
    def encode(self, emb: torch.Tensor, n_q: Optional[int] = None) -> torch.Tensor:
        """ResidualVectorQuantization.encode (core_vq.py): per codebook the nearest entry of the running residual.
        emb float32 [B, 128, T] -> codes int64 [n_q, B, T].  The distance search -(|x|^2 - 2 x.E + |E|^2) is one float32
        GEMM per codebook (2 x.E with -|E|^2 as its bias; |x|^2 does not change the argmax)."""
        if self._rt is None:
            self._rt = GemmRuntime("f32", self.device)
            self._neg_sq = (-(self.tables ** 2).sum(-1)).contiguous()          # [n_q][bins]
        rt = self._rt
        src = emb.device
        B, D, T = emb.shape
        nq = self.tables.shape[0] if n_q is None else n_q
        bins = self.tables.shape[1]
        res = emb.to(self.device, torch.float32).transpose(1, 2).reshape(B * T, D).contiguous()
        scores = torch.empty((B * T, bins), dtype=torch.float32, device=self.device)
        out = []
        for q in range(nq):
            rt.gemm(operand(res.data_ptr(), D, 1), operand(self.tables[q].data_ptr(), D, 1), scores.data_ptr(), B * T, bins, D,
                    dtype=L.F32, ldc_m=bins, bias=self._neg_sq[q], alpha=2.0)
            idx = scores.argmax(dim=-1)
            res = res - self.tables[q][idx]
            out.append(idx.view(B, T))
        return torch.stack(out).to(src)

    @torch.no_grad()
    def quantize(self, emb: torch.Tensor, n_q: Optional[int] = None, *, codes: bool = True, latents: bool = True):
        """``encode`` and ``decode`` of the result in ONE launch (jen1_rvq_encode): emb float32 [B, 128, T] -> (codes int64 [n_q, B, T] or
        None, latents float32 [B, 128, T] or None), both on the quantizer's device.  The latents are bit-identical to ``decode(codes)``.  No
        host synchronisation: the call can be captured in a graph."""
        if not (codes or latents):
            raise ValueError("quantize: nothing asked for (codes=False, latents=False)")
        B, D, T = emb.shape
        nq = self.tables.shape[0] if n_q is None else n_q
        c = torch.empty((nq, B, T), dtype=torch.int64, device=self.device) if codes else None
        z = torch.empty((B, D, T), dtype=torch.float32, device=self.device) if latents else None
        self.quantize_into(emb, nq, c, z, B, 0)
        return c, z

    @torch.no_grad()
    def quantize_into(self, emb: torch.Tensor, n_q: Optional[int], codes: Optional[torch.Tensor], latents: Optional[torch.Tensor], B_out: int,
                      t0: int) -> None:
        """the same into a time slot of preallocated outputs: emb [rows, 128, T] holds rows / B_out segments of B_out batch rows each (row
        j B_out + b, as ``EncodecHIP.segment_rows`` orders them), which land side by side from frame ``t0`` of codes int64 [n_q, B_out, T']
        and / or latents float32 [B_out, 128, T'] (contiguous, on the quantizer's device)"""
        rows, D, T = emb.shape
        nq = self.tables.shape[0] if n_q is None else n_q
        assert 1 <= nq <= self.tables.shape[0]
        bins = self.tables.shape[1]
        x = emb.to(self.device, torch.float32).contiguous()
        for o, dt in ((codes, torch.int64), (latents, torch.float32)):
            assert o is None or (o.is_contiguous() and o.dtype == dt and o.device == x.device), "outputs must be contiguous on the quantizer's device"
        assert codes is None or tuple(codes.shape[:2]) == (nq, B_out)
        assert latents is None or tuple(latents.shape[:2]) == (B_out, D)
        s = torch.cuda.current_stream(self.device).cuda_stream
        L.check(self.lib.jen1_rvq_encode(x.data_ptr(), self.tables.data_ptr(), self.e_sq.data_ptr(), None if codes is None else codes.data_ptr(),
                                         None if latents is None else latents.data_ptr(), nq, rows, T, bins, D, B_out,
                                         0 if codes is None else codes.shape[2], t0, 0 if latents is None else latents.shape[2], t0, s),
                "jen1_rvq_encode")

    @torch.no_grad()
    def decode(self, codes: torch.Tensor) -> torch.Tensor:
        """codes int64 [n_q', B, T] (n_q' <= n_q) -> float32 [B, 128, T] on the codes' device"""
        src = codes.device
        c = codes.to(self.device, torch.int64).contiguous()
        nq, B, T = c.shape
        assert nq <= self.tables.shape[0]
        bins, D = self.tables.shape[1], self.tables.shape[2]
        out = torch.empty((B, D, T), dtype=torch.float32, device=self.device)
        s = torch.cuda.current_stream(self.device).cuda_stream
        L.check(self.lib.jen1_rvq_decode(c.data_ptr(), self.tables.data_ptr(), out.data_ptr(), nq, B, T, bins, D, s), "jen1_rvq_decode")
        return out.to(src)


class _SEANetOps:
    """the building blocks both halves of the SEANet share (encodec modules/conv.py, modules/lstm.py, modules/seanet.py)"""

    def __init__(self, params: Dict[str, torch.Tensor], lstm_name: str, compute_dtype: str, device):
        self.rt = GemmRuntime(compute_dtype, device)
        self.device = self.rt.device
        self.p = {k: v.detach().to(self.device, torch.float32).contiguous() for k, v in params.items()}
        assert "layers.0.norm.weight" in self.p, "only the 48 kHz model's norm='time_group_norm' is built (no weight_norm)"
        assert f"{lstm_name}.lstm.weight_ih_l0" in self.p, f"{lstm_name} must be the LSTM"
        self.lstm_name = lstm_name
        self.n_lstm = 0
        while f"{lstm_name}.lstm.weight_ih_l{self.n_lstm}" in self.p:
            self.n_lstm += 1
        dt = self.rt.tdtype
        # LSTM operands: W_ih as a linear weight (packed by the runtime), W_hh transposed [H][4H], the two biases summed
        self.whh_t = [self.p[f"{lstm_name}.lstm.weight_hh_l{l}"].t().contiguous().to(dt) for l in range(self.n_lstm)]
        self.whh = [self.p[f"{lstm_name}.lstm.weight_hh_l{l}"].to(dt).contiguous() for l in range(self.n_lstm)]
        # jen1_lstm_layer_multi (register-resident W_hh over H / 32 workgroups, one grid barrier per step) unless disabled
        self.lstm_multi = os.environ.get("JEN1_LSTM_MULTI", "1") == "1"
        self.last_lstm_counters: Optional[torch.Tensor] = None
        self._lstm_flags: List[torch.Tensor] = []
        self.lstm_bias = [(self.p[f"{lstm_name}.lstm.bias_ih_l{l}"] + self.p[f"{lstm_name}.lstm.bias_hh_l{l}"]).contiguous()
                          for l in range(self.n_lstm)]

    def _check_lstm(self) -> None:
        """raise if a grid barrier of the multi-workgroup LSTM timed out (its workgroups were not co-resident)"""
        flags, self._lstm_flags = self._lstm_flags, []
        if flags and int(torch.stack([f[:, 1].sum() for f in flags]).sum()) != 0:
            raise L.Jen1HipError("jen1_lstm_layer_multi: grid barrier time-out (workgroups not co-resident); set JEN1_LSTM_MULTI=0")

    def _to_rows(self, x_bct: torch.Tensor) -> torch.Tensor:
        B, C, T = x_bct.shape
        h = torch.zeros((B, T, pad8(C)), dtype=self.rt.tdtype, device=self.device)
        h[:, :, :C] = x_bct.transpose(1, 2)
        return h

    # ------------------------------------------------------------------ building blocks
    def _norm(self, x: torch.Tensor, name: str, C: int) -> torch.Tensor:
        rt, lib = self.rt, self.rt.lib
        B, Lx, ld = x.shape
        sums = torch.empty((B, 1, 2), dtype=torch.float32, device=x.device)
        y = (torch.zeros_like if ld != C else torch.empty_like)(x)
        s = rt.stream()
        dt = rt.dt_of(x)
        L.check(lib.jen1_gn_sums(x.data_ptr(), sums.data_ptr(), B, Lx, C, ld, 1, dt, s), "jen1_gn_sums")
        L.check(lib.jen1_gn_apply(x.data_ptr(), sums.data_ptr(), self.p[f"{name}.norm.weight"].data_ptr(), self.p[f"{name}.norm.bias"].data_ptr(),
                                  None, 0, y.data_ptr(), B, Lx, C, ld, 1, 1e-5, 0, dt, s), "jen1_gn_apply")
        return y

    def _pad1d(self, x: torch.Tensor, left: int, right: int) -> torch.Tensor:
        """``pad1d(x, (left, right), "reflect")`` of modules/conv.py as an explicit copy (jen1_codec_pad1d), small-input rule included"""
        B, Lx, ld = x.shape
        y = torch.empty((B, Lx + left + right, ld), dtype=x.dtype, device=x.device)
        L.check(self.rt.lib.jen1_codec_pad1d(x.data_ptr(), y.data_ptr(), B, Lx, ld, left, right, self.rt.dt_of(x), self.rt.stream()), "jen1_codec_pad1d")
        return y

    def _conv(self, x: torch.Tensor, name: str, stride: int = 1, tiny: bool = False) -> torch.Tensor:
        """SConv1d, non-causal: reflect padding of k - stride (split right-first) plus the extra right padding that
        makes the frame count whole (modules/conv.py get_extra_padding_for_conv1d), conv, GroupNorm(1).
        An input of no more frames than the padding is outside what the index map of the GEMM can mirror; ``tiny=True`` (what the two
        networks pass) applies pad1d's small-input rule through a padded copy of those few frames, ``tiny=False`` refuses them."""
        w, b = self.p[f"{name}.conv.weight"], self.p[f"{name}.conv.bias"]
        co, ci, k = w.shape
        Lx = x.shape[1]
        total = k - stride
        left = total - total // 2
        Lout = -(-(Lx - k + total) // stride) + 1                  # ceil((L - k + total) / stride) + 1
        right = (Lout - 1) * stride + k - left - Lx                # total // 2 + extra padding
        if Lx <= max(left, right):
            if not tiny:
                raise NotImplementedError(f"{name}: {Lx} frames are not more than the reflect padding ({left}, {right}); pass tiny=True for "
                                          "the small-input case of encodec's pad1d")
            x = self._pad1d(x.contiguous(), left, right)
            g = ConvGeom("conv", k, stride, 0, Lx + left + right, Lout, ci, co)
        else:
            g = ConvGeom("conv", k, stride, left, Lx, Lout, ci, co, reflect=True)
        y = conv_forward(self.rt, x, self.rt.packed(w, "conv", x.dtype), b, g)
        return self._norm(y, name, co)

    def _conv_transpose(self, x: torch.Tensor, name: str, stride: int) -> torch.Tensor:
        """SConvTranspose1d, non-causal: full transposed conv, GroupNorm(1) over the UNtrimmed length, then trim"""
        w, b = self.p[f"{name}.conv.weight"], self.p[f"{name}.conv.bias"]
        ci, co, k = w.shape
        Lx = x.shape[1]
        full = (Lx - 1) * stride + k
        g = ConvGeom("convT", k, stride, 0, Lx, full, ci, co)
        y = self._norm(conv_forward(self.rt, x, self.rt.packed(w, "convT", x.dtype), b, g), name, co)
        total = k - stride
        right = total // 2
        return y[:, total - right: full - right].contiguous()

    def _elu(self, x: torch.Tensor) -> torch.Tensor:
        y = torch.empty_like(x)
        L.check(self.rt.lib.jen1_act_forward(x.data_ptr(), y.data_ptr(), x.numel(), 2, self.rt.dt_of(x), self.rt.stream()), "jen1_act_forward")
        return y

    def _resblock(self, x: torch.Tensor, name: str) -> torch.Tensor:
        h = self._conv(self._elu(x), f"{name}.block.1", tiny=True)
        h = self._conv(self._elu(h), f"{name}.block.3", tiny=True)
        return self._conv(x, f"{name}.shortcut", tiny=True) + h

    def lstm_multi_rows(self) -> int:
        """the most sequences one pass may hold for ``_lstm`` to stay on jen1_lstm_layer_multi (its co-residency bound)"""
        H = self.whh[0].shape[1]
        return 8 * (256 // (H // 32))

    def _lstm(self, x: torch.Tensor) -> torch.Tensor:
        """SLSTM: y = LSTM(x) + x over the time axis (modules/lstm.py)"""
        rt = self.rt
        B, T, H = x.shape
        dt = rt.dt_of(x)
        h = x
        for l in range(self.n_lstm):
            wih = rt.packed(self.p[f"{self.lstm_name}.lstm.weight_ih_l{l}"], "linear", x.dtype)
            gin = torch.empty((B, T, 4 * H), dtype=torch.float32, device=x.device)
            rt.gemm(operand(h.data_ptr(), h.shape[-1], 1), operand(wih.data_ptr(), wih.shape[-1], 1), gin.data_ptr(), B * T, 4 * H, H,
                    dtype=dt, ldc_m=4 * H, bias=self.lstm_bias[l], c_f32=True)
            y = torch.empty_like(x)
            last = l == self.n_lstm - 1
            groups = (B + 7) // 8
            if self.lstm_multi and groups * (H // 32) <= 256:
                hbuf = torch.empty((groups, 2, 16, H), dtype=torch.float32, device=x.device)
                cnt = torch.zeros((groups, 32), dtype=torch.int32, device=x.device)
                L.check(rt.lib.jen1_lstm_layer_multi(gin.data_ptr(), self.whh[l].data_ptr(), x.data_ptr() if last else None, y.data_ptr(),
                                                     hbuf.data_ptr(), cnt.data_ptr(), B, T, H, y.shape[-1], dt, rt.stream()),
                        "jen1_lstm_layer_multi")
                self.last_lstm_counters = cnt        # cnt[:, 1] != 0 reports a barrier time-out (checked in _check_lstm)
                self._lstm_flags.append(cnt)
            else:
                L.check(rt.lib.jen1_lstm_layer(gin.data_ptr(), self.whh_t[l].data_ptr(), x.data_ptr() if last else None, y.data_ptr(), B, T, H,
                                               y.shape[-1], dt, rt.stream()), "jen1_lstm_layer")
            h = y
        return h



class SEANetDecoderHIP(_SEANetOps):
    def __init__(self, params: Dict[str, torch.Tensor], ratios: Sequence[int] = (8, 5, 4, 2), n_residual_layers: int = 1,
                 compute_dtype: str = "bf16", device="cuda"):
        super().__init__(params, "layers.1", compute_dtype, device)
        self.ratios, self.n_res = list(ratios), n_residual_layers
        idx = 2
        self.stages: List[tuple] = []
        for r in self.ratios:
            self.stages.append((idx + 1, r, [idx + 2 + j for j in range(self.n_res)]))
            idx += 2 + self.n_res
        self.last = idx + 1
        assert f"layers.{self.last}.conv.weight" in self.p, f"expected the output convolution at layers.{self.last}"

    @classmethod
    def from_module(cls, decoder: torch.nn.Module, ratios: Sequence[int] = (8, 5, 4, 2), **kw) -> "SEANetDecoderHIP":
        """from a ``transformers`` EncodecDecoder (its state_dict already uses the key names this class reads)"""
        return cls({k: v for k, v in decoder.state_dict().items()}, ratios, **kw)

    # ------------------------------------------------------------------ SEANetDecoder.forward
    @property
    def channels(self) -> int:
        return self.p[f"layers.{self.last}.conv.weight"].shape[0]

    @torch.no_grad()
    def rows(self, emb: torch.Tensor) -> torch.Tensor:
        """latents [B, 128, T] on the decoder's device -> the output convolution's rows as it leaves them: channel-last
        [B, hop * T, pad8(channels)] in the compute dtype (what jen1_codec_overlap_add reads); the caller runs ``_check_lstm``"""
        h = self._conv(self._to_rows(emb.to(self.device, torch.float32)), "layers.0", tiny=True)
        h = self._lstm(h)
        for conv_idx, ratio, res in self.stages:
            h = self._conv_transpose(self._elu(h), f"layers.{conv_idx}", ratio)
            for r in res:
                h = self._resblock(h, f"layers.{r}")
        return self._conv(self._elu(h), f"layers.{self.last}", tiny=True)

    @torch.no_grad()
    def __call__(self, emb: torch.Tensor) -> torch.Tensor:
        """latents [B, 128, T] (any device) -> audio float32 [B, channels, hop * T] on the same device"""
        src = emb.device
        h = self.rows(emb)
        out = h[:, :, :self.channels].to(torch.float32).transpose(1, 2).contiguous().to(src)
        self._check_lstm()
        return out


class SEANetEncoderHIP(_SEANetOps):
    """encodec modules/seanet.py::SEANetEncoder, 48 kHz settings: conv k7, then per ratio (reversed: 2, 4, 5, 8) a residual
    block, ELU and a strided conv (k = 2 r); LSTM; ELU; conv k7 to the 128 latent channels"""

    def __init__(self, params: Dict[str, torch.Tensor], ratios: Sequence[int] = (8, 5, 4, 2), n_residual_layers: int = 1,
                 compute_dtype: str = "bf16", device="cuda"):
        n_stage = len(ratios) * (n_residual_layers + 2)
        super().__init__(params, f"layers.{1 + n_stage}", compute_dtype, device)
        self.ratios, self.n_res = list(reversed(list(ratios))), n_residual_layers
        self.last = 1 + n_stage + 2
        assert f"layers.{self.last}.conv.weight" in self.p, f"expected the output convolution at layers.{self.last}"

    @classmethod
    def from_module(cls, encoder: torch.nn.Module, ratios: Sequence[int] = (8, 5, 4, 2), **kw) -> "SEANetEncoderHIP":
        return cls({k: v for k, v in encoder.state_dict().items()}, ratios, **kw)

    @torch.no_grad()
    def __call__(self, audio: torch.Tensor) -> torch.Tensor:
        """audio [B, channels, L] -> latents float32 [B, 128, ceil(L / 320)] on the same device"""
        src = audio.device
        out = self.from_rows(self._to_rows(audio.to(self.device, torch.float32))).to(src)
        self._check_lstm()
        return out

    @torch.no_grad()
    def from_rows(self, rows: torch.Tensor) -> torch.Tensor:
        """the same from the first convolution's input rows [B, L, pad8(channels)] in the compute dtype (jen1_codec_segment_cut writes
        them) -> latents float32 [B, 128, ceil(L / 320)] on the encoder's device; the caller runs ``_check_lstm``"""
        h = self._conv(rows, "layers.0", tiny=True)
        idx = 1
        for r in self.ratios:
            for j in range(self.n_res):
                h = self._resblock(h, f"layers.{idx + j}")
            idx += self.n_res
            h = self._conv(self._elu(h), f"layers.{idx + 1}", stride=r, tiny=True)
            idx += 2
        h = self._lstm(h)
        h = self._conv(self._elu(h), f"layers.{self.last}", tiny=True)
        ch = self.p[f"layers.{self.last}.conv.weight"].shape[0]
        return h[:, :, :ch].to(torch.float32).transpose(1, 2).contiguous()


def segment_lengths(n: int, segment_length: int, segment_stride: int) -> List[int]:
    """the sample counts of the segments ``EncodecModel.encode`` cuts ``n`` samples into (model.py: one per offset 0, stride, ...)"""
    return [min(segment_length, n - off) for off in range(0, n, segment_stride)]


def segment_frame_counts(n: int, segment_length: int, segment_stride: int, hop: int = HOP_48K) -> List[int]:
    """the latent frames per segment, ceil(samples / hop): 10 s at 48 kHz -> 10 x 150 + 15"""
    return [-(-m // hop) for m in segment_lengths(n, segment_length, segment_stride)]


def _runs(values: Sequence[int]) -> List[tuple]:
    """(first index, count, value) of every run of equal neighbours"""
    out: List[tuple] = []
    for i, v in enumerate(values):
        if out and out[-1][2] == v:
            out[-1] = (out[-1][0], out[-1][1] + 1, v)
        else:
            out.append((i, 1, v))
    return out


class EncodecHIP:
    """the slice of ``EncodecModel`` generation.py touches: ``.channels``, ``.sample_rate``, ``.quantizer.decode``,
    ``.decoder``, ``.encode`` -- and the codec's own way back, which the reference leaves out: ``.decode`` / ``.decode_latents``
    (per-segment decoder, x scale, linear overlap-add)"""

    def __init__(self, decoder: SEANetDecoderHIP, quantizer: ResidualVectorQuantizerHIP, channels: int = 2, sample_rate: int = 48000,
                 encode: Optional[Callable] = None, encoder: Optional["SEANetEncoderHIP"] = None, segment: float = 1.0,
                 overlap: float = 0.01, normalize: bool = True, n_q: Optional[int] = None):
        self.decoder, self.quantizer, self.channels, self.sample_rate, self._encode = decoder, quantizer, channels, sample_rate, encode
        self.encoder, self.normalize, self.n_q = encoder, normalize, n_q
        self.decoder_device = decoder.device       # Jen1.generate hands the sampled latents over where they are (no host round trip)
        self.segment_length = int(segment * sample_rate)                                   # encodec model.py segment_length
        self.segment_stride = max(1, int((1 - overlap) * self.segment_length))             # encodec model.py segment_stride
        # JEN1_ENCODE_BATCHED=0: one encoder pass per segment, scales and cut in torch (the form before the segment kernels; the A/B)
        self.encode_batched = os.environ.get("JEN1_ENCODE_BATCHED", "1") == "1"

    def segment_frames(self, n_samples: int) -> List[int]:
        """latent frames per segment for ``n_samples`` of audio: the layout ``encode`` produces and ``decode_latents`` undoes"""
        return segment_frame_counts(n_samples, self.segment_length, self.segment_stride)

    @torch.no_grad()
    def encode(self, audio: torch.Tensor):
        """``EncodecModel.encode`` of the package (model.py): the audio is cut into 1 s segments with 1 % overlap, every
        segment is normalised by the RMS of its mono mix, encoded and quantised with ALL codebooks (the reference never
        sets a target bandwidth) -> ``[(codes [B, n_q, T_seg], scale [B, 1]), ...]``, which is what ``get_emb``
        concatenates (generation.py:145-150; dataloader.py:106-114).  Segments of equal length share one encoder pass
        (``_encode_batched``); JEN1_ENCODE_BATCHED=0 keeps one pass per segment."""
        if self._encode is not None:
            return self._encode(audio)
        if self.encoder is None:
            raise NotImplementedError("no encoder: construct EncodecHIP with encoder=SEANetEncoderHIP(...) or encode=<callable>")
        assert audio.dim() == 3 and 0 < audio.shape[1] <= 2
        if self.encode_batched:
            return self._encode_batched(audio)
        frames = []
        for offset in range(0, audio.shape[-1], self.segment_stride):
            x = audio[:, :, offset: offset + self.segment_length]
            scale = None
            if self.normalize:
                mono = x.mean(dim=1, keepdim=True)
                scale = 1e-8 + mono.pow(2).mean(dim=2, keepdim=True).sqrt()
                x = x / scale
                scale = scale.view(-1, 1)
            codes = self.quantizer.encode(self.encoder(x), self.n_q).transpose(0, 1)       # [B, n_q, T]
            frames.append((codes, scale))
        return frames

    def segment_scales(self, audio: torch.Tensor) -> torch.Tensor:
        """audio float32 [B, C, N] on the encoder's device -> the per-segment scale [B, S] (jen1_codec_segment_scales)"""
        enc = self.encoder
        B, C, N = audio.shape
        S = len(segment_lengths(N, self.segment_length, self.segment_stride))
        scale = torch.empty((B, S), dtype=torch.float32, device=enc.device)
        L.check(enc.rt.lib.jen1_codec_segment_scales(audio.data_ptr(), scale.data_ptr(), B, C, N, self.segment_length, self.segment_stride, S,
                                                     enc.rt.stream()), "jen1_codec_segment_scales")
        return scale

    def segment_rows(self, audio: torch.Tensor, scale: Optional[torch.Tensor], s0: int, n_sel: int, length: int) -> torch.Tensor:
        """the encoder's input rows [n_sel * B, length, 8] (row j * B + b) of the equal-length segments s0 .. s0 + n_sel - 1, divided by
        their scales when given (jen1_codec_segment_cut)"""
        enc = self.encoder
        B, C, N = audio.shape
        S = len(segment_lengths(N, self.segment_length, self.segment_stride))
        rows = torch.empty((n_sel * B, length, pad8(C)), dtype=enc.rt.tdtype, device=enc.device)
        L.check(enc.rt.lib.jen1_codec_segment_cut(audio.data_ptr(), None if scale is None else scale.data_ptr(), rows.data_ptr(), B, C, N, length,
                                                  self.segment_stride, S, s0, n_sel, enc.rt.dt_of(rows), enc.rt.stream()), "jen1_codec_segment_cut")
        return rows

    def _encode_batched(self, audio: torch.Tensor):
        enc = self.encoder
        src = audio.device
        x = audio.to(enc.device, torch.float32).contiguous()
        B = x.shape[0]
        scale = self.segment_scales(x) if self.normalize else None
        per_pass = max(1, enc.lstm_multi_rows() // B)              # more rows would push _lstm off the multi-workgroup kernel
        frames: List[tuple] = []
        for s0, count, length in _runs(segment_lengths(x.shape[-1], self.segment_length, self.segment_stride)):
            for j0 in range(0, count, per_pass):
                n = min(per_pass, count - j0)
                emb = enc.from_rows(self.segment_rows(x, scale, s0 + j0, n, length))                    # [n B, 128, T]
                codes = self.quantizer.encode(emb, self.n_q)                                             # [n_q, n B, T]
                for j in range(n):
                    s = s0 + j0 + j
                    frames.append((codes[:, j * B:(j + 1) * B].transpose(0, 1).to(src), None if scale is None else scale[:, s:s + 1].to(src)))
        enc._check_lstm()
        return frames

    @torch.no_grad()
    def encode_latents(self, audio: torch.Tensor):
        """``encode`` followed by the quantizer's decode of all segments, without the codes in between: audio [B, C, N] -> (latents
        float32 [B, 128, T'] with the segments side by side in time, the frame count of every segment, the per-segment scales [B, S] or
        None), on the audio's device -- what ``Jen1.get_emb_segments`` returns.  The passes are those of ``_encode_batched``; the search of
        every pass (jen1_rvq_encode) writes its latents straight into their time slot of the result."""
        if self.encoder is None:
            raise NotImplementedError("no encoder: construct EncodecHIP with encoder=SEANetEncoderHIP(...)")
        assert audio.dim() == 3 and 0 < audio.shape[1] <= 2
        enc = self.encoder
        src = audio.device
        x = audio.to(enc.device, torch.float32).contiguous()
        B = x.shape[0]
        counts = self.segment_frames(x.shape[-1])
        offs = [sum(counts[:s]) for s in range(len(counts))]
        scale = self.segment_scales(x) if self.normalize else None
        per_pass = max(1, enc.lstm_multi_rows() // B)
        out = torch.empty((B, 128, sum(counts)), dtype=torch.float32, device=self.quantizer.device)
        for s0, count, length in _runs(segment_lengths(x.shape[-1], self.segment_length, self.segment_stride)):
            for j0 in range(0, count, per_pass):
                n = min(per_pass, count - j0)
                emb = enc.from_rows(self.segment_rows(x, scale, s0 + j0, n, length))                    # [n B, 128, T]
                assert emb.shape[2] == counts[s0 + j0]
                self.quantizer.quantize_into(emb, self.n_q, None, out, B, offs[s0 + j0])
        enc._check_lstm()
        return out.to(src), counts, None if scale is None else scale.to(src)

    # ------------------------------------------------------------------ EncodecModel.decode
    @torch.no_grad()
    def decode(self, frames) -> torch.Tensor:
        """``EncodecModel.decode`` of the package (model.py): ``[(codes [B, n_q, T_s], scale [B, 1] or None), ...]`` -> audio
        ``[B, channels, stride (S - 1) + 320 T_last]`` on the codes' device: per-frame decoder, x scale, ``_linear_overlap_add``.  One
        jen1_rvq_decode call looks up the codes of all frames."""
        assert len(frames) > 0, "no frames"
        src = frames[0][0].device
        codes = torch.cat([c.to(self.decoder_device) for c, _ in frames], dim=-1).permute(1, 0, 2)       # [n_q, B, sum T_s]
        emb = self.quantizer.decode(codes)
        scales = None
        if any(s is not None for _, s in frames):
            B = codes.shape[1]
            dev = self.decoder_device
            scales = torch.cat([torch.ones((B, 1), device=dev) if s is None else s.reshape(B, 1).to(dev, torch.float32) for _, s in frames], dim=1)
        return self.decode_latents(emb, [int(c.shape[-1]) for c, _ in frames], scales).to(src)

    @torch.no_grad()
    def decode_latents(self, emb: torch.Tensor, segment_frames: Sequence[int], scales: Optional[torch.Tensor] = None,
                       length: Optional[int] = None) -> torch.Tensor:
        """the same for continuous latents ``[B, 128, T']`` that hold the segments side by side (what ``get_emb`` builds and the sampler
        returns): ``segment_frames`` is the frame count of every segment (``segment_frames(n_samples)`` of the encode that defined the
        layout), ``scales`` ``[B, S]`` or None (unit), ``length`` trims the audio to that many samples.  Segments of equal length go through
        the decoder together as batch rows (row j B + b), at most as many per pass as keep its LSTM on the multi-workgroup kernel; the
        overlap-add reads the decoder's final rows in place (jen1_codec_overlap_add)."""
        dec = self.decoder
        src = emb.device
        counts = [int(t) for t in segment_frames]
        S = len(counts)
        if emb.dim() != 3 or S == 0 or min(counts) < 1 or sum(counts) != emb.shape[2]:
            raise ValueError(f"segment_frames {counts} do not add up to the {tuple(emb.shape)} latents")
        if max(counts) != counts[0]:
            raise ValueError("the first segment must be the longest (its length defines the overlap-add weights)")
        B = emb.shape[0]
        total = self.segment_stride * (S - 1) + HOP_48K * counts[-1]
        n_out = total if length is None else int(length)
        if not 1 <= n_out <= total:
            raise ValueError(f"length={length} is outside what the {S} segments cover ({total} samples)")
        if any(HOP_48K * t < self.segment_stride for t in counts[:-1]):
            raise ValueError(f"segment_frames {counts}: a segment before the last is shorter than the stride of {self.segment_stride} samples, "
                             "which leaves samples no segment covers")
        if scales is not None and tuple(scales.shape) != (B, S):
            raise ValueError(f"scales must be [B, S] = {(B, S)}, not {tuple(scales.shape)}")
        x = emb.to(dec.device, torch.float32)
        offs = [sum(counts[:s]) for s in range(S)]
        per_pass = max(1, dec.lstm_multi_rows() // B)
        by_len: Dict[int, List[int]] = {}
        for s, t in enumerate(counts):
            by_len.setdefault(t, []).append(s)
        table: List[Optional[tuple]] = [None] * S                 # per segment: (the pass's rows, first row, samples)
        for t, segs in by_len.items():
            for j0 in range(0, len(segs), per_pass):
                part = segs[j0:j0 + per_pass]
                rows = dec.rows(torch.cat([x[:, :, offs[s]:offs[s] + t] for s in part], dim=0))            # [n B, 320 t, 8]
                for j, s in enumerate(part):
                    table[s] = (rows, j * B, HOP_48K * t)
        segs_d = L.ola_seg_table([(r.data_ptr(), r0, n) for r, r0, n in table], dec.device)
        sc = None if scales is None else scales.to(dec.device, torch.float32).contiguous()
        out = torch.empty((B, dec.channels, n_out), dtype=torch.float32, device=dec.device)
        L.check(dec.rt.lib.jen1_codec_overlap_add(segs_d.data_ptr(), S, None if sc is None else sc.data_ptr(), out.data_ptr(), B, dec.channels,
                                                  table[0][0].shape[-1], n_out, self.segment_stride, HOP_48K * counts[0], HOP_48K * counts[-1],
                                                  dec.rt.dt_of(table[0][0]), dec.rt.stream()), "jen1_codec_overlap_add")
        dec._check_lstm()
        return out.to(src)
