"""Frechet Audio Distance on libjen1_hip.so: the Frechet distance between Gaussian fits of VGGish embeddings of two sets of clips
(Kilgour et al., "Frechet Audio Distance", 2019), the figure the JEN-1 paper reports.  Not in the reference, which has no evaluation.

  front end   ``convert_audio`` to 16 kHz mono, ``jen1_mel`` with VGGish's framing (periodic Hann of 400 samples, hop 160, FFT 512,
              magnitude, no centre padding) and VGGish's mel matrix (``vggish_mel_matrix``: 64 bands, 125..7500 Hz, triangles linear in
              mel), ``log(mel + 0.01)``, non-overlapping examples of 96 frames.  The resampler is this package's windowed-sinc filter,
              not the ``resampy`` of the original pipeline.
  embedder    csrc/vggish.hip (include/jen1_fad.h): the first layer on the vector ALU (it reads ``jen1_mel``'s output and applies the
              log itself), five 3x3 convolutions as implicit GEMMs on the exact-float32 matrix instructions with bias, ReLU and the 2x2
              max-pool in the epilogue, three linears on ``jen1_train_gemm`` (float32; the last one writes the embeddings transposed,
              where ``jen1_latent_moments`` reads them).  The weights are an input (``VGGishHIP.from_state_dict``): the keys of the
              common PyTorch port, widths taken from the shapes.
  statistics  ``FrechetStats`` keeps count, sum and sum of outer products in float64 on the device (``jen1_latent_moments``, the state
              of ``normalizer.state_words``); ``frechet_distance`` works on the host in float64.

No autograd (inputs that require grad are refused), no CPU path (``Jen1HipError`` off the GPU), no torchaudio, no ``conv2d``.  The
PCA / quantisation post-processor of VGGish is not part of FAD and is not here.
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import audio_host as H
from . import lib as L
from . import spectral
from .normalizer import latent_moments, state_words

SR = 16000
N_FFT, HOP, WIN = 512, 160, 400
FRAMES, BANDS = 96, 64
MEL_LO_HZ, MEL_HI_HZ = 125.0, 7500.0
LOG_OFFSET = 0.01
PAD = (N_FFT - WIN) // 2            # jen1_mel centres the window in the frame: 56 zeros in front put frame k on samples [160 k, 160 k + 400)
CONV_KEYS = ("features.0", "features.3", "features.6", "features.8", "features.11", "features.13")
POOL_AFTER = (True, True, False, True, False, True)
LINEAR_KEYS = ("embeddings.0", "embeddings.2", "embeddings.4")
GRID = ((96, 64), (48, 32), (24, 16), (24, 16), (12, 8), (12, 8))       # H x W at the input of every convolution
FLAT_HW = 6 * 4
CHUNK = 256                         # examples per pass of the network (bounds the activations; results do not depend on it)


# ------------------------------------------------------------------------------------------------------------- front end
def vggish_mel_matrix() -> np.ndarray:
    """float64 [64, 257]: VGGish's mel matrix on the bins ``linspace(0, 8000, 257)``.  ``mel(f) = 1127 ln(1 + f / 700)``; 66 edges equally
    spaced in mel from mel(125) to mel(7500); band i is ``max(0, min((m - lo) / (c - lo), (hi - m) / (hi - c)))`` at a bin of mel value m
    -- triangles linear in MEL (``spectral.mel_filterbank``'s are linear in Hz).  The DC column is zero."""
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)
    m = mel(np.linspace(0.0, SR / 2.0, N_FFT // 2 + 1))
    edges = np.linspace(mel(MEL_LO_HZ), mel(MEL_HI_HZ), BANDS + 2)
    lo, c, hi = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    w = np.maximum(0.0, np.minimum((m[None, :] - lo) / (c - lo), (hi - m[None, :]) / (hi - c)))
    w[:, 0] = 0.0
    return w


def example_count(n_samples_16k: int) -> int:
    """examples of a 16 kHz signal of that many samples: ``(1 + (n - 400) // 160) // 96``, 0 below 400 samples"""
    n = int(n_samples_16k)
    return 0 if n < WIN else (1 + (n - WIN) // HOP) // FRAMES


def _check_float(t, what: str) -> None:
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise TypeError(f"{what}: float32 tensors, not {getattr(t, 'dtype', type(t))}")
    if t.requires_grad:
        raise ValueError(f"{what}: a metric, not a loss -- there is no autograd; detach the input")


def vggish_bands(dev: torch.device) -> H.Bands:
    return H.device_table(dev, ("vggish",), lambda: H.Bands.on(dev, *spectral.banded(vggish_mel_matrix())))


def _mel(wav: torch.Tensor, sr: int, lengths, what: str):
    """wav [..., C, L] at ``sr`` -> (linear mel [rows, 64, frames] or None when no row holds a frame, counts per row, frames)"""
    from . import audio
    _check_float(wav, what)
    if wav.dim() < 2 or int(wav.shape[-1]) < 1:
        raise ValueError(f"{what}: audio is [..., C, L], not {tuple(wav.shape)}")
    dev = H.gpu_device(wav.device, what)
    x = audio.convert_audio(wav, int(sr), SR, 1, device=dev)
    n16 = int(x.shape[-1])
    x = x.reshape(-1, n16)
    rows = int(x.shape[0])
    if lengths is None:
        counts = [example_count(n16)] * rows
    else:
        vals = H.host_ints(lengths, rows, f"{what}: lengths")
        if any(v < 0 or v > int(wav.shape[-1]) for v in vals):
            raise ValueError(f"{what}: lengths must lie in 0..{int(wav.shape[-1])}")
        # samples beyond a row's length are taken as padding: a resampled row is as long as convert_audio would make the cut row
        counts = [example_count(-(-v * SR // int(sr))) for v in vals]
    if n16 < WIN or sum(counts) == 0:
        return None, counts, 0
    xp = torch.nn.functional.pad(x, (PAD, PAD))
    n = n16 + 2 * PAD
    fr = H.framing(N_FFT, HOP, WIN, "hann", False, n=n)
    mel = torch.empty((rows, BANDS, fr.frames), dtype=torch.float32, device=dev)
    H.launch(dev, "jen1_mel", xp.data_ptr(), n, mel.data_ptr(), *H.frame_tables(fr, "hann", dev), *vggish_bands(dev).abi(), *fr.abi(rows, n),
             L.SPEC_MAGNITUDE, L.SPEC_LOG_NONE, 0.0)
    return mel, counts, fr.frames


def vggish_examples(wav: torch.Tensor, sr: int, device="cuda", lengths=None) -> Tuple[torch.Tensor, List[int]]:
    """wav float32 [..., C, L] (C in {1, 2}) on a GPU at rate ``sr`` -> (log-mel examples float32 [N_total, 96, 64], examples per row).
    ``lengths`` (host integers, one per row, in samples at ``sr``): rows padded to a common L count only up to their own length.  A
    row shorter than one example gives none."""
    mel, counts, frames = _mel(wav, sr, lengths, "vggish_examples")
    total = sum(counts)
    out = torch.empty((total, FRAMES, BANDS), dtype=torch.float32, device=wav.device)
    if total:
        H.launch(wav.device, "jen1_vggish_examples", mel.data_ptr(), H.c_ints(counts), len(counts), frames, out.data_ptr())
    return out, counts


# ------------------------------------------------------------------------------------------------------------- weights
def pack_conv3x3(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 3, 3] -> the flat float32 layout of ``jen1_conv3x3`` (include/jen1_fad.h): [G][Q][tap][c4][nt][k][j] with
    cout = 64 g + 16 nt + j, cin = 16 q + 4 c4 + k, zeros beyond Cout"""
    co, ci = int(w.shape[0]), int(w.shape[1])
    G, Q = -(-co // 64), ci // 16
    full = torch.zeros((G * 64, ci, 9), dtype=torch.float32)
    full[:co] = w.detach().to("cpu", torch.float32).reshape(co, ci, 9)
    return full.reshape(G, 4, 16, Q, 4, 4, 9).permute(0, 3, 6, 4, 1, 5, 2).contiguous().reshape(-1)      # g nt j q c4 k tap -> g q tap c4 nt k j


def unpack_conv3x3(packed: torch.Tensor, cin: int, cout: int) -> torch.Tensor:
    """the inverse of ``pack_conv3x3``: [cout, cin, 3, 3]"""
    G, Q = -(-cout // 64), cin // 16
    full = packed.detach().to("cpu").reshape(G, Q, 9, 4, 4, 4, 16).permute(0, 4, 6, 1, 3, 5, 2).reshape(G * 64, cin, 3, 3)
    return full[:cout].contiguous()


def _channels_ok(c: int) -> bool:
    return 16 <= c <= 512 and c % 16 == 0


class VGGishHIP:
    """The VGGish embedding network on the HIP kernels.  ``from_state_dict`` takes the tensors; ``forward`` / ``embed`` need a GPU."""

    def __init__(self):
        raise TypeError("use VGGishHIP.from_state_dict or VGGishHIP.from_module")

    @classmethod
    def from_state_dict(cls, sd, final_relu: bool = False, device="cuda") -> "VGGishHIP":
        """``sd``: ``features.{0,3,6,8,11,13}.{weight,bias}`` ([Cout, Cin, 3, 3]) and ``embeddings.{0,2,4}.{weight,bias}``; the widths come from
        the shapes (multiples of 16 up to 512 for the channels, an embedding of a multiple of 16 up to 128).  ``final_relu``: keep an
        activation after the last linear, as some ports do (FAD is defined without it)."""
        self = object.__new__(cls)
        self.final_relu = bool(final_relu)
        self.device = torch.device(device)
        get = lambda k: _tensor(sd, k)
        self.channels: List[int] = []
        self.conv_w, self.conv_b = [], []
        cin = 1
        for key in CONV_KEYS:
            w, b = get(key + ".weight"), get(key + ".bias")
            if w.dim() != 4 or tuple(w.shape[1:]) != (cin, 3, 3) or not _channels_ok(int(w.shape[0])):
                raise ValueError(f"{key}.weight: shape {tuple(w.shape)}, expected [Cout, {cin}, 3, 3] with Cout a multiple of 16 in 16..512")
            if tuple(b.shape) != (int(w.shape[0]),):
                raise ValueError(f"{key}.bias: shape {tuple(b.shape)}, expected [{int(w.shape[0])}]")
            cout = int(w.shape[0])
            packed = w.reshape(cout, 9).t().contiguous() if cin == 1 else pack_conv3x3(w)      # the first layer: [tap][Cout]
            self.conv_w.append(packed.to(self.device))
            self.conv_b.append(b.contiguous().to(self.device))
            self.channels.append(cout)
            cin = cout
        self.lin_w, self.lin_b, self.widths = [], [], []
        k = FLAT_HW * cin
        for key in LINEAR_KEYS:
            w, b = get(key + ".weight"), get(key + ".bias")
            if w.dim() != 2 or int(w.shape[1]) != k or int(w.shape[0]) % 16 != 0 or int(w.shape[0]) < 16:
                raise ValueError(f"{key}.weight: shape {tuple(w.shape)}, expected [out, {k}] with out a multiple of 16")
            if tuple(b.shape) != (int(w.shape[0]),):
                raise ValueError(f"{key}.bias: shape {tuple(b.shape)}, expected [{int(w.shape[0])}]")
            self.lin_w.append(w.contiguous().to(self.device))
            self.lin_b.append(b.contiguous().to(self.device))
            k = int(w.shape[0])
            self.widths.append(k)
        self.dim = k
        if self.dim > 128:
            raise ValueError(f"{LINEAR_KEYS[-1]}.weight: an embedding of {self.dim} values, at most 128 fit the statistics kernel")
        self._rt = None
        return self

    @classmethod
    def from_module(cls, m, final_relu: bool = False, device="cuda") -> "VGGishHIP":
        """anything whose ``state_dict()`` has the keys of ``from_state_dict``"""
        return cls.from_state_dict(m.state_dict(), final_relu=final_relu, device=device)

    def packed_state(self) -> dict:
        """the tensors as the kernels read them (tests unpack them with ``unpack_conv3x3``)"""
        return {"conv_w": self.conv_w, "conv_b": self.conv_b, "lin_w": self.lin_w, "lin_b": self.lin_b}

    # ------------------------------------------------------------------ the network
    def _runtime(self):
        from .gemm_host import GemmRuntime
        H.gpu_device(self.device, "VGGishHIP")
        if self._rt is None:
            self._rt = GemmRuntime("f32", self.device)
        return self._rt

    def _convs(self, first_layer, n: int) -> torch.Tensor:
        """the six convolutions on ``n`` examples whose first layer ``first_layer(y)`` writes [n, 48, 32, C1]: [n, 6 * 4 * C4], the
        (h, w, c) order the first linear expects (NHWC needs no permutation)"""
        dev = self.device
        x = torch.empty((n, 48, 32, self.channels[0]), dtype=torch.float32, device=dev)
        first_layer(x)
        for i in range(1, 6):
            h, w = GRID[i]
            pool = POOL_AFTER[i]
            cin, cout = self.channels[i - 1], self.channels[i]
            y = torch.empty((n, h // 2 if pool else h, w // 2 if pool else w, cout), dtype=torch.float32, device=dev)
            H.launch(dev, "jen1_conv3x3", x.data_ptr(), self.conv_w[i].data_ptr(), self.conv_b[i].data_ptr(), y.data_ptr(), n, h, w, cin, cout,
                     int(pool))
            x = y
        return x.reshape(n, -1)

    def _linears(self, x: torch.Tensor, out_t: torch.Tensor, col0: int) -> None:
        """the three linears on x [n, K]; the embeddings go to ``out_t[:, col0 : col0 + n]`` (out_t: [dim, N_total])"""
        from .gemm_host import operand
        rt = self._runtime()
        n = int(x.shape[0])
        for j, (w, b) in enumerate(zip(self.lin_w, self.lin_b)):
            K, nout = int(w.shape[1]), int(w.shape[0])
            # one route for every batch size (the plain 64 x 64 tiles, no split over K): a row's sums do not depend on the batch.
            # The last linear writes [dim][N_total]: element (example m, value c) at c N_total + col0 + m.
            if j == len(self.lin_w) - 1:
                rt.gemm(operand(x.data_ptr(), K, 1), operand(w.data_ptr(), K, 1, tap_stride=nout * K), out_t.data_ptr() + 4 * col0, n, nout, K,
                        dtype=L.F32, ldc_m=1, ldc_n=int(out_t.shape[1]), bias=b)
            else:
                y = torch.empty((n, nout), dtype=torch.float32, device=self.device)
                rt.gemm(operand(x.data_ptr(), K, 1), operand(w.data_ptr(), K, 1, tap_stride=nout * K), y.data_ptr(), n, nout, K, dtype=L.F32,
                        ldc_m=nout, bias=b)
                H.launch(self.device, "jen1_vggish_relu", y.data_ptr(), y.numel())
                x = y

    def _embed(self, src: torch.Tensor, counts: List[int], frames: int, is_log: int, out_t: torch.Tensor) -> None:
        """the network over the ``sum(counts)`` examples of ``src`` (rows of ``frames`` frames holding ``counts[r]`` examples each; ``is_log``:
        log-mel examples, not ``jen1_mel``'s linear output), CHUNK at a time, into ``out_t``"""
        host = H.c_ints(counts)
        for n0 in range(0, int(out_t.shape[1]), CHUNK):
            n = min(CHUNK, int(out_t.shape[1]) - n0)
            first = lambda y, n0=n0, n=n: H.launch(self.device, "jen1_vggish_conv1", src.data_ptr(), host, len(counts), frames, is_log, n0, n,
                                                   self.conv_w[0].data_ptr(), self.conv_b[0].data_ptr(), y.data_ptr(), self.channels[0])
            self._linears(self._convs(first, n), out_t, n0)

    def _finish(self, out_t: torch.Tensor) -> torch.Tensor:
        if self.final_relu and out_t.numel():
            H.launch(self.device, "jen1_vggish_relu", out_t.data_ptr(), out_t.numel())
        return out_t.t()                           # [N, dim], a view: the memory stays [dim][N], what the statistics read

    @torch.no_grad()
    def forward(self, examples: torch.Tensor) -> torch.Tensor:
        """log-mel examples float32 [N, 96, 64] on the GPU -> embeddings float32 [N, dim] (a transposed view of [dim, N])"""
        _check_float(examples, "VGGishHIP.forward")
        H.gpu_device(examples.device, "VGGishHIP.forward")
        if examples.dim() != 3 or tuple(examples.shape[1:]) != (FRAMES, BANDS) or int(examples.shape[0]) < 1:
            raise ValueError(f"VGGishHIP.forward: examples are [N, {FRAMES}, {BANDS}] with N >= 1, not {tuple(examples.shape)}")
        self._runtime()
        ex = examples.to(self.device).contiguous()
        N = int(ex.shape[0])
        out_t = torch.empty((self.dim, N), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._embed(ex, [1] * N, FRAMES, 1, out_t)
            return self._finish(out_t)

    __call__ = forward

    @torch.no_grad()
    def embed(self, wav: torch.Tensor, sr: int, lengths=None) -> Tuple[torch.Tensor, List[int]]:
        """wav float32 [..., C, L] on the GPU at rate ``sr`` -> (embeddings [N_total, dim], examples per row).  The first layer reads the
        mel spectrogram where ``jen1_mel`` left it: the examples are never written."""
        self._runtime()
        mel, counts, frames = _mel(wav, sr, lengths, "VGGishHIP.embed")
        N = sum(counts)
        out_t = torch.empty((self.dim, N), dtype=torch.float32, device=self.device)
        if N == 0:
            return out_t.t(), counts
        with torch.cuda.device(self.device):
            self._embed(mel, counts, frames, 0, out_t)
            return self._finish(out_t), counts


def _tensor(sd, key: str) -> torch.Tensor:
    if key not in sd:
        raise KeyError(f"the VGGish state dict has no {key!r}")
    t = sd[key]
    if not torch.is_tensor(t) or not t.dtype.is_floating_point:
        raise ValueError(f"{key}: a floating-point tensor is needed, not {getattr(t, 'dtype', type(t))}")
    return t.detach().to("cpu", torch.float32)


# ------------------------------------------------------------------------------------------------------------- statistics
class FrechetStats:
    """Count, sum and sum of outer products of embeddings, float64 ``[1 + C + C C]`` (``normalizer.state_words``), filled on the device by
    ``jen1_latent_moments``; mean and covariance on the host in float64."""

    def __init__(self, dim: int = 128):
        dim = int(dim)
        if dim < 16 or dim > 128 or dim % 16 != 0:
            raise ValueError(f"dim = {dim}: the statistics kernel takes a multiple of 16 in 16..128")
        self.dim = dim
        self.state = torch.zeros(state_words(dim), dtype=torch.float64)

    @torch.no_grad()
    def update(self, emb: torch.Tensor) -> "FrechetStats":
        """add the rows of ``emb`` float32 [N, dim] on a GPU (N = 0 adds nothing).  A transposed view of a [dim, N] tensor -- what
        ``VGGishHIP`` returns -- is read in place; anything else is copied into that layout first."""
        _check_float(emb, "FrechetStats.update")
        H.gpu_device(emb.device, "FrechetStats.update")
        if emb.dim() != 2 or int(emb.shape[1]) != self.dim:
            raise ValueError(f"FrechetStats.update: embeddings are [N, {self.dim}], not {tuple(emb.shape)}")
        N = int(emb.shape[0])
        if N == 0:
            return self
        z = emb.t()
        if not z.is_contiguous():
            z = z.contiguous()                     # the transpose copy: embeddings that did not come from VGGishHIP
        self.state = latent_moments(z[None], None, self.state)
        return self

    @torch.no_grad()
    def merge(self, other: "FrechetStats") -> "FrechetStats":
        """add the statistics of ``other``: the states are sums, so the result is the fit over both sets"""
        if other.dim != self.dim:
            raise ValueError(f"cannot merge statistics of {other.dim} values into statistics of {self.dim}")
        self.state += other.state.to(self.state.device)
        return self

    def all_reduce(self, group=None) -> "FrechetStats":
        """SUM all-reduce of the state over ``group``"""
        import torch.distributed as dist
        dist.all_reduce(self.state, op=dist.ReduceOp.SUM, group=group)
        return self

    def _host(self) -> np.ndarray:
        return self.state.detach().to("cpu", torch.float64).numpy()

    @property
    def count(self) -> int:
        return int(round(float(self.state[0])))

    def mean(self) -> np.ndarray:
        s = self._host()
        if s[0] < 1:
            raise ValueError("no embeddings: there is no mean")
        return s[1:1 + self.dim] / s[0]

    def cov(self) -> np.ndarray:
        """the unbiased covariance (n - 1), as ``numpy.cov`` and the published FAD tools; float64 [dim, dim], symmetric"""
        s = self._host()
        n = s[0]
        if n < 2:
            raise ValueError(f"{int(n)} embeddings are too few for a covariance: at least 2 are needed")
        mu = s[1:1 + self.dim] / n
        c = (s[1 + self.dim:].reshape(self.dim, self.dim) - n * np.outer(mu, mu)) / (n - 1.0)
        return 0.5 * (c + c.T)

    def state_dict(self) -> dict:
        return {"dim": self.dim, "state": self.state.detach().to("cpu").clone()}

    def load_state_dict(self, sd) -> "FrechetStats":
        if int(sd["dim"]) != self.dim:
            raise ValueError(f"the saved statistics have {sd['dim']} values per embedding, these {self.dim}")
        if tuple(sd["state"].shape) != tuple(self.state.shape):
            raise ValueError(f"state: shape {tuple(sd['state'].shape)} in the file, {tuple(self.state.shape)} here")
        self.state = sd["state"].detach().to(self.state.device, torch.float64).clone()
        return self

    @classmethod
    def from_state_dict(cls, sd) -> "FrechetStats":
        return cls(int(sd["dim"])).load_state_dict(sd)


def _sym_root(S: np.ndarray) -> np.ndarray:
    lam, U = np.linalg.eigh(S)
    return (U * np.sqrt(np.maximum(lam, 0.0))) @ U.T


def frechet_distance(a: FrechetStats, b: FrechetStats) -> float:
    """``|mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr (S_a S_b)^(1/2)`` on the host in float64.  The last trace is the sum of the square roots of
    the eigenvalues of ``R S_b R``, ``R = S_a^(1/2)`` from ``eigh`` with negative eigenvalues clamped to 0: every matrix stays symmetric, and a
    rank-deficient fit (fewer embeddings than dimensions) stays real and finite.  Those square roots are taken as the singular values of
    ``S_b^(1/2) R`` -- ``R S_b R = (S_b^(1/2) R)^T (S_b^(1/2) R)`` -- which are the same numbers without the loss of a root: an eigenvalue
    that should be 0 comes out as ``eps lambda_max^2`` and its root as ``sqrt(eps) lambda_max``, over a hundred of them in a fit of 18
    embeddings, where a singular value that should be 0 comes out as ``eps sigma_max``."""
    if a.dim != b.dim:
        raise ValueError(f"the sets have embeddings of {a.dim} and {b.dim} values")
    if a.count < 2 or b.count < 2:
        raise ValueError(f"a Frechet distance needs at least 2 embeddings per set, not {a.count} and {b.count}")
    mu_a, mu_b, Sa, Sb = a.mean(), b.mean(), a.cov(), b.cov()
    sigma = np.linalg.svd(_sym_root(Sb) @ _sym_root(Sa), compute_uv=False)
    d = mu_a - mu_b
    return float(d @ d + np.trace(Sa) + np.trace(Sb) - 2.0 * sigma.sum())


class FrechetAudioDistance:
    """``stats`` embeds a set of clips and fits it; ``score`` is the distance between two sets.  A reference set is embedded once,
    saved with ``FrechetStats.state_dict()`` and reused for every checkpoint."""

    def __init__(self, model: VGGishHIP):
        self.model = model

    def _batches(self, wavs, sr) -> Iterable[Tuple[torch.Tensor, int]]:
        if torch.is_tensor(wavs):
            if sr is None:
                raise ValueError("a tensor of clips needs its sample rate")
            yield wavs, int(sr)
            return
        for item in wavs:
            if torch.is_tensor(item):
                if sr is None:
                    raise ValueError("a list of clips needs its sample rate")
                yield item, int(sr)
            else:
                w, r = item
                yield w, int(r)

    @torch.no_grad()
    def stats(self, wavs, sr: Optional[int] = None) -> FrechetStats:
        """``wavs``: one tensor [..., C, L], a list of tensors of any lengths (``sr`` for all), or an iterable of ``(wav, sr)`` batches.
        Raises when the set holds no full example (0.975 s at 16 kHz)."""
        st = FrechetStats(self.model.dim)
        for w, r in self._batches(wavs, sr):
            emb, _ = self.model.embed(w, r)
            st.update(emb)
        if st.count == 0:
            raise ValueError("the set holds no full example: every clip is shorter than 96 frames (15 600 samples at 16 kHz)")
        return st

    def score(self, test, reference, sr: Optional[int] = None) -> float:
        """the distance of ``test`` from ``reference``; either side may be a ready ``FrechetStats``"""
        a = test if isinstance(test, FrechetStats) else self.stats(test, sr)
        b = reference if isinstance(reference, FrechetStats) else self.stats(reference, sr)
        return frechet_distance(a, b)
