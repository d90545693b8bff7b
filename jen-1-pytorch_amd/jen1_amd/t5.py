"""The text side of the conditioning on libjen1_hip.so: token ids -> the ``(emb, mask)`` pair of ``T5Conditioner.forward``.

Host side of csrc/t5.hip (C ABI: include/jen1_t5.h).  ``T5EncoderHIP`` is the encoder stack of ``transformers.T5EncoderModel`` in eval
mode (reference jen1/conditioners.py:61-105 runs ``google/flan-t5-large`` in float32 on stock operators); ``T5ConditionerHIP`` wraps
it the way ``T5Conditioner`` + ``MultiConditioner`` do (conditioners.py:84-111, :182-208) and is a valid ``conditioner=`` of ``Jen1``.
The tokenizer stays the caller's (a SentencePiece model on the CPU, no arithmetic).

Per block (8 launches; 8 L + 2 for the stack):
    n   = rmsnorm(h += wo-output of the block before)    jen1_t5_rmsnorm       h: float32 residual stream in every mode
    qkv = n [q | k | v]^T                                jen1_train_gemm       one stacked projection
    a   = softmax(q k^T + bias, key mask) v              jen1_t5_attention     matrix cores, one launch for all heads
    d   = a o^T                                          jen1_train_gemm       float32 output
    n   = rmsnorm(h += d)                                jen1_t5_rmsnorm
    u   = n [wi_0 | wi_1]^T   (or n wi^T)                jen1_train_gemm
    g   = gelu_new(u_0) * u_1 (or relu(u))               jen1_t5_gate
    d   = g wo^T                                         jen1_train_gemm       float32 output
then ``final_layer_norm`` of h += d.  The whole stack is captured as one graph per (B, N) through ``graphs.capture``.

The relative-position bias is a host-built ``[heads, 2 N - 1]`` table per sequence length: ``table[h, (j - i) + N - 1] =
relative_attention_bias.weight[bucket(j - i), h]`` with the buckets computed by torch float32 operations in Hugging Face's order
(distances 16, 32 and 64 sit exactly on boundaries of the logarithm; tests/golden/t5_encoder.npz pins them).
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from .gemm_host import GemmRuntime, operand, want_skinny

EPS = 1e-6                      # T5Config.layer_norm_epsilon
MAX_DISTANCE = 128              # T5Config.relative_attention_max_distance
BLOCK = "encoder.block.{}.layer.{}."
REL_BIAS = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"


class T5Geometry(NamedTuple):
    vocab: int
    d_model: int
    heads: int
    d_kv: int
    d_ff: int
    layers: int
    buckets: int
    gated: bool

    @property
    def inner(self) -> int:
        return self.heads * self.d_kv


def infer_geometry(shapes: Dict[str, Sequence[int]]) -> T5Geometry:
    """the geometry of a ``T5EncoderModel.state_dict()`` from the shapes of its entries ({key: shape})"""
    for k in ("shared.weight", REL_BIAS, "encoder.final_layer_norm.weight"):
        if k not in shapes:
            raise KeyError(f"not a T5EncoderModel state_dict: {k} is missing")
    vocab, d_model = (int(s) for s in shapes["shared.weight"])
    buckets, heads = (int(s) for s in shapes[REL_BIAS])
    layers = 0
    while BLOCK.format(layers, 0) + "SelfAttention.q.weight" in shapes:
        layers += 1
    if layers == 0:
        raise KeyError("not a T5EncoderModel state_dict: no encoder.block.0")
    inner = int(shapes[BLOCK.format(0, 0) + "SelfAttention.q.weight"][0])
    if inner % heads != 0:
        raise ValueError(f"q.weight has {inner} rows, not a multiple of the {heads} heads of the bias table")
    ff = BLOCK.format(0, 1) + "DenseReluDense."
    gated = ff + "wi_0.weight" in shapes
    d_ff = int(shapes[ff + ("wi_0.weight" if gated else "wi.weight")][0])
    return T5Geometry(vocab, d_model, heads, inner // heads, d_ff, layers, buckets, gated)


def relative_position_bucket(relative_position: torch.Tensor, num_buckets: int = 32, max_distance: int = MAX_DISTANCE) -> torch.Tensor:
    """``T5Attention._relative_position_bucket(bidirectional=True)``: the same torch float32 operations in the same order"""
    num_buckets //= 2
    buckets = (relative_position > 0).to(torch.long) * num_buckets
    relative_position = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    if_large = max_exact + (torch.log(relative_position.float() / max_exact) / math.log(max_distance / max_exact)
                            * (num_buckets - max_exact)).to(torch.long)
    if_large = torch.min(if_large, torch.full_like(if_large, num_buckets - 1))
    return buckets + torch.where(is_small, relative_position, if_large)


def bias_table(rel_bias_weight: torch.Tensor, N: int, max_distance: int = MAX_DISTANCE) -> torch.Tensor:
    """float32 ``[heads, 2 N - 1]`` on the CPU: entry ``[h, r + N - 1]`` is the bias a query adds to the key ``r = j - i`` places behind it"""
    w = rel_bias_weight.detach().to("cpu", torch.float32)
    rel = torch.arange(-(N - 1), N, dtype=torch.long)
    return w[relative_position_bucket(rel, w.shape[0], max_distance)].t().contiguous()


def check_mask(attention_mask: torch.Tensor) -> None:
    """Hugging Face adds finfo.min to padded keys; leaving them out is the same thing as long as a row keeps one token"""
    if attention_mask.dim() != 2:
        raise ValueError(f"attention_mask must be [B, N], not {tuple(attention_mask.shape)}")
    if not bool((attention_mask != 0).any(dim=1).all()):
        raise ValueError("attention_mask has a row without a single token: softmax over no keys is undefined")


class _Buffers:
    def __init__(self, enc: "T5EncoderHIP", B: int, N: int):
        g, dev, td = enc.geo, enc.device, enc.rt.tdtype
        M = B * N
        f32 = dict(dtype=torch.float32, device=dev)
        self.B, self.N, self.M = B, N, M
        self.ids = torch.zeros(M, dtype=torch.int64, device=dev)
        self.mask = torch.ones((B, N), dtype=torch.int32, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.h = torch.zeros((M, g.d_model), **f32)
        self.delta = torch.zeros((M, g.d_model), **f32)
        self.out = torch.zeros((M, g.d_model), **f32)
        self.n = torch.zeros((M, g.d_model), dtype=td, device=dev)
        self.qkv = torch.zeros((M, 3 * g.inner), dtype=td, device=dev)
        self.att = torch.zeros((M, g.inner), dtype=td, device=dev)
        self.u = torch.zeros((M, (2 if g.gated else 1) * g.d_ff), dtype=td, device=dev)
        self.g = torch.zeros((M, g.d_ff), dtype=td, device=dev)
        self.bias = bias_table(enc.rel_bias, N).to(dev)
        self.graph: Optional[torch.cuda.CUDAGraph] = None


class T5EncoderHIP:
    """``T5EncoderModel`` (encoder stack, eval mode) on the HIP path.  ``compute_dtype``: what the linears and the attention read and
    write, "f32" (default: the reference runs the encoder with autocast disabled, conditioners.py:102) or "bf16"; the residual stream, the
    norms' statistics and the softmax are float32 in both."""

    def __init__(self, sd: Dict[str, torch.Tensor], compute_dtype: str = "f32", device="cuda", act: Optional[str] = None):
        from . import lib as L
        geo = infer_geometry({k: tuple(v.shape) for k, v in sd.items()})
        act = act or ("gelu_new" if geo.gated else "relu")
        if (geo.gated, act) not in ((True, "gelu_new"), (False, "relu")):
            raise ValueError(f"unsupported feed-forward: gated={geo.gated} with act={act!r} (gated gelu_new and plain relu are built)")
        if geo.d_kv not in (16, 32, 64):
            raise ValueError(f"d_kv = {geo.d_kv}: jen1_t5_attention takes 16, 32 or 64")
        if geo.d_model % 8 or geo.d_ff % 8:
            raise ValueError(f"d_model = {geo.d_model} and d_ff = {geo.d_ff} must be multiples of 8")
        self.L, self.geo, self.act = L, geo, act
        self.rt = rt = GemmRuntime(compute_dtype, device)
        self.device, self.compute_dtype = rt.device, compute_dtype
        dev, td = rt.device, rt.tdtype

        def w32(key: str) -> torch.Tensor:
            return sd[key].detach().to(dev, torch.float32).contiguous()

        def stacked(keys: List[str]) -> torch.Tensor:
            ws = [w32(k) for k in keys]
            mat, _ = rt.packed_bank(ws, [torch.zeros(w.shape[0], device=dev) for w in ws], td)
            return mat[0]

        self.shared = w32("shared.weight")
        self.rel_bias = sd[REL_BIAS].detach().to("cpu", torch.float32)
        self.final_ln = w32("encoder.final_layer_norm.weight")
        self.blocks = []
        for i in range(geo.layers):
            a, f = BLOCK.format(i, 0), BLOCK.format(i, 1)
            wo_a, wo_f = w32(a + "SelfAttention.o.weight"), w32(f + "DenseReluDense.wo.weight")
            blk = {"ln0": w32(a + "layer_norm.weight"), "ln1": w32(f + "layer_norm.weight"),
                   "qkv": stacked([a + f"SelfAttention.{n}.weight" for n in "qkv"]),
                   "o": rt.packed(wo_a, "linear", td)[0], "wo": rt.packed(wo_f, "linear", td)[0]}
            if geo.gated:
                blk["wi"] = stacked([f + "DenseReluDense.wi_0.weight", f + "DenseReluDense.wi_1.weight"])
            else:
                blk["wi"] = rt.packed(w32(f + "DenseReluDense.wi.weight"), "linear", td)[0]
            self.blocks.append(blk)
        self._bufs: Dict[Tuple[int, int], _Buffers] = {}
        self.launches = 0                # of the last recorded / eager pass

    @classmethod
    def from_state_dict(cls, sd: Dict[str, torch.Tensor], compute_dtype: str = "f32", device="cuda", act: Optional[str] = None) -> "T5EncoderHIP":
        """``sd``: ``T5EncoderModel.state_dict()`` (tensors or arrays).  The geometry is read from the shapes; ``act`` None: gelu_new for
        the gated feed-forward (flan-t5), relu for the plain one (t5)."""
        return cls({k: torch.as_tensor(v) for k, v in sd.items()}, compute_dtype, device, act)

    @classmethod
    def from_module(cls, hf_model, compute_dtype: str = "f32", device="cuda") -> "T5EncoderHIP":
        """from a ``transformers.T5EncoderModel`` (or the full model: only ``shared`` and ``encoder.*`` are read)"""
        cfg = hf_model.config
        if float(cfg.layer_norm_epsilon) != EPS or int(cfg.relative_attention_max_distance) != MAX_DISTANCE:
            raise ValueError("layer_norm_epsilon / relative_attention_max_distance differ from the T5 defaults this path is built for")
        act = {"gelu_new": "gelu_new", "relu": "relu"}.get(cfg.dense_act_fn)
        if act is None:
            raise ValueError(f"dense_act_fn = {cfg.dense_act_fn!r} is not built")
        sd = {k: v for k, v in hf_model.state_dict().items() if k == "shared.weight" or k.startswith("encoder.")}
        return cls.from_state_dict(sd, compute_dtype, device, act)

    # ------------------------------------------------------------------ the pass
    def _linear(self, x: torch.Tensor, w: torch.Tensor, out: torch.Tensor) -> None:
        """out[M][n] = x[M][K] w[n][K]^T; a float32 ``out`` in bf16 mode is the GEMM's float32 epilogue"""
        M, K = x.shape
        n = w.shape[0]
        assert w.shape[1] == K and out.shape == (M, n)
        rt = self.rt
        rt.gemm(operand(x.data_ptr(), K, 1), operand(w.data_ptr(), K, 1, tap_stride=n * K), out.data_ptr(), M, n, K, dtype=rt.dt,
                ldc_m=n, c_f32=out.dtype == torch.float32 and rt.tdtype != torch.float32, skinny=want_skinny(rt, M, n, (K + 31) // 32))
        self.launches += 1

    def _norm(self, b: _Buffers, add: Optional[torch.Tensor], weight: torch.Tensor, y: torch.Tensor) -> None:
        L = self.L
        L.check(self.rt.lib.jen1_t5_rmsnorm(b.h.data_ptr(), None if add is None else add.data_ptr(), weight.data_ptr(), y.data_ptr(), b.M,
                                            self.geo.d_model, EPS, L.F32 if y.dtype == torch.float32 else L.BF16, self.rt.stream()), "jen1_t5_rmsnorm")
        self.launches += 1

    def _run(self, b: _Buffers) -> None:
        L, rt, g = self.L, self.rt, self.geo
        lib, st = rt.lib, rt.stream()
        self.launches = 1
        L.check(lib.jen1_t5_embed(b.ids.data_ptr(), self.shared.data_ptr(), b.h.data_ptr(), b.err.data_ptr(), b.M, g.vocab, g.d_model, st), "jen1_t5_embed")
        for i, blk in enumerate(self.blocks):
            self._norm(b, b.delta if i > 0 else None, blk["ln0"], b.n)
            self._linear(b.n, blk["qkv"], b.qkv)
            L.check(lib.jen1_t5_attention(b.qkv.data_ptr(), 3 * g.inner, b.att.data_ptr(), g.inner, b.bias.data_ptr(), b.mask.data_ptr(), b.B, g.heads,
                                          b.N, g.d_kv, rt.dt, st), "jen1_t5_attention")
            self._linear(b.att, blk["o"], b.delta)
            self._norm(b, b.delta, blk["ln1"], b.n)
            self._linear(b.n, blk["wi"], b.u)
            L.check(lib.jen1_t5_gate(b.u.data_ptr(), b.g.data_ptr(), b.M, g.d_ff, L.T5_ACT_GELU_NEW if g.gated else L.T5_ACT_RELU, rt.dt, st), "jen1_t5_gate")
            self._linear(b.g, blk["wo"], b.delta)
            self.launches += 2
        self._norm(b, b.delta, self.final_ln, b.out)

    @torch.no_grad()
    def __call__(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, graph: bool = True) -> torch.Tensor:
        """``last_hidden_state``: float32 [B, N, d_model].  ``graph=False`` issues the launches one by one instead of replaying the
        captured graph of this (B, N)."""
        if input_ids.dim() != 2 or tuple(attention_mask.shape) != tuple(input_ids.shape):
            raise ValueError(f"input_ids {tuple(input_ids.shape)} and attention_mask {tuple(attention_mask.shape)} must both be [B, N]")
        B, N = input_ids.shape
        if not 1 <= N <= self.L.T5_MAX_TOKENS:
            raise ValueError(f"N = {N}: jen1_t5_attention takes 1 .. {self.L.T5_MAX_TOKENS} tokens")
        check_mask(attention_mask)
        b = self._bufs.get((B, N))
        if b is None:
            b = self._bufs[(B, N)] = _Buffers(self, B, N)
        b.ids.copy_(input_ids.reshape(-1).to(torch.int64))
        b.mask.copy_((attention_mask != 0).to(torch.int32))
        if not graph:
            self._run(b)
        else:
            if b.graph is None:
                from .graphs import capture
                self._run(b)                 # warm-up: every kernel is loaded and its LDS attribute set before the capture
                torch.cuda.synchronize(self.device)
                gr = torch.cuda.CUDAGraph()
                with capture(gr):
                    self._run(b)
                b.graph = gr
            b.graph.replay()
        out = b.out.view(B, N, self.geo.d_model).clone()
        if int(b.err.item()) != 0:
            b.err.zero_()
            raise self.L.Jen1HipError(f"jen1_t5_embed: input_ids hold an id outside the table of {self.geo.vocab} rows")
        return out


class T5ConditionerHIP:
    """``T5Conditioner`` (conditioners.py:32-111) with the encoder and the projection on the HIP path, and at the same time the
    ``MultiConditioner`` around it (conditioners.py:182-208): ``conditioner(batch_metadata, device) -> {id: (emb, mask)}``.

    ``tokenizer``: the caller's (``AutoTokenizer.from_pretrained(...)``), called exactly as the reference calls it.  ``encoder``:
    ``T5EncoderHIP`` (anything with ``(input_ids, attention_mask) -> [B, N, F]``).  ``proj_weight`` [out, F] / ``proj_bias`` [out]: the
    reference's ``proj_out``.  The last ``cache_size`` prompt tuples are kept: the three conditioner calls of a trainer micro-batch with
    repeated prompts (trainer.py:183-213), or repeated ``generate()`` calls with one prompt, cost one pass."""

    def __init__(self, tokenizer, encoder, proj_weight: torch.Tensor, proj_bias: torch.Tensor, max_length: int = 128, id: str = "prompt", *,
                 dtype: str = "f32", cache_size: int = 4, tail=None):
        self.tokenizer, self.encoder, self.max_length, self.id = tokenizer, encoder, int(max_length), id
        self.proj_weight, self.proj_bias, self.dtype = proj_weight, proj_bias, dtype
        self.cache_size = int(cache_size)
        self._tail = tail                # (input: a projection + mask multiply other than TextConditionerTail, for tests without a GPU)
        self._cache: "OrderedDict[tuple, Tuple[torch.Tensor, torch.Tensor]]" = OrderedDict()
        self.hits = self.misses = 0

    def _tail_on(self, device):
        if self._tail is None:
            from .tasks import TextConditionerTail
            self._tail = TextConditionerTail(self.proj_weight, self.proj_bias, dtype=self.dtype, device=device)
        return self._tail

    @torch.no_grad()
    def forward(self, texts: Sequence[str], device) -> Tuple[torch.Tensor, torch.Tensor]:
        """conditioners.py:84-111: (embeddings [B, max_length, out] float32 with padded tokens zeroed, attention_mask [B, max_length] bool)"""
        key = (tuple(texts), str(device))
        hit = self._cache.get(key)
        if hit is not None:
            self._cache.move_to_end(key)
            self.hits += 1
            return hit[0].clone(), hit[1].clone()
        self.misses += 1
        encoded = self.tokenizer(list(texts), truncation=True, max_length=self.max_length, padding="max_length", return_tensors="pt")
        check_mask(encoded["attention_mask"])                                    # (on the CPU: no device round trip)
        input_ids = encoded["input_ids"].to(device)
        attention_mask = encoded["attention_mask"].to(device).to(torch.bool)
        hidden = self.encoder(input_ids, attention_mask)
        emb, _ = self._tail_on(device)(hidden, attention_mask)
        self._cache[key] = (emb, attention_mask)
        while len(self._cache) > self.cache_size:
            self._cache.popitem(last=False)
        return emb.clone(), attention_mask.clone()

    def __call__(self, batch_metadata: Sequence[dict], device) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        """conditioners.py:182-208 for the one conditioner this object is"""
        texts = []
        for x in batch_metadata:
            if self.id not in x:
                raise ValueError(f"Conditioner key {self.id} not found in batch metadata")
            v = x[self.id]
            # (the reference unwraps lists of any length and one-element tuples: collation functions wrap everything in a list)
            texts.append(v[0] if isinstance(v, list) or (isinstance(v, tuple) and len(v) == 1) else v)
        return {self.id: self.forward(texts, device)}
