"""Float64 torch restatement of the T5 encoder stack (transformers.T5EncoderModel, eval mode) and of the arithmetic of each kernel of
csrc/t5.hip, shared by tests/test_t5_host.py (CPU: the restatement against the Hugging Face fixture) and tests/test_gpu_t5.py (GPU: the
kernels and the captured encoder against the restatement).  ``encoder(..., dtype=torch.float32 / torch.bfloat16)`` is the same stack on
stock torch operators in that dtype: the baseline of tools/t5_bench.py.
"""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jen-1-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from jen1_amd.init_fill import fill, fill_uniform  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "t5_encoder.npz")
SEED = 1234
EPS = 1e-6
CASES = ("tiny-gated", "tiny-relu", "wide")
BLOCK = "encoder.block.{}.layer.{}."
REL_BIAS = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"


def schema_of(vocab, d_model, heads, d_kv, d_ff, layers, gated, buckets=32):
    """[(key, shape)] of ``T5EncoderModel.state_dict()`` (the tied ``encoder.embed_tokens.weight`` left out)"""
    inner = heads * d_kv
    s = [("shared.weight", (vocab, d_model))]
    for i in range(layers):
        a, f = BLOCK.format(i, 0), BLOCK.format(i, 1)
        s += [(a + f"SelfAttention.{n}.weight", (inner, d_model)) for n in "qkv"]
        s.append((a + "SelfAttention.o.weight", (d_model, inner)))
        if i == 0:
            s.append((REL_BIAS, (buckets, heads)))
        s.append((a + "layer_norm.weight", (d_model,)))
        s += [(f + f"DenseReluDense.{n}.weight", (d_ff, d_model)) for n in (("wi_0", "wi_1") if gated else ("wi",))]
        s += [(f + "DenseReluDense.wo.weight", (d_model, d_ff)), (f + "layer_norm.weight", (d_model,))]
    s.append(("encoder.final_layer_norm.weight", (d_model,)))
    return s


# the fixture's cases: geometry, batch, tokens, kept tokens per row, stored channel step
CASE_SPECS = {
    "tiny-gated": dict(geo=dict(vocab=96, d_model=64, heads=4, d_kv=16, d_ff=96, layers=2, gated=True), B=2, N=24, lengths=(24, 8), step=1),
    "tiny-relu": dict(geo=dict(vocab=96, d_model=64, heads=4, d_kv=32, d_ff=96, layers=2, gated=False), B=2, N=24, lengths=(24, 8), step=1),
    "wide": dict(geo=dict(vocab=512, d_model=1024, heads=16, d_kv=64, d_ff=2816, layers=2, gated=True), B=2, N=128, lengths=(128, 1), step=8),
}


def case_inputs(case, variant=0):
    """(input_ids [B, N] int64, attention_mask [B, N] int64) of a fixture case; ``variant`` > 0: other ids and masks of the same shape"""
    spec = CASE_SPECS[case]
    B, N, vocab = spec["B"], spec["N"], spec["geo"]["vocab"]
    tag = f"t5.{case}.ids" + ("" if variant == 0 else f".v{variant}")
    ids = np.minimum((fill_uniform(tag, (B, N), SEED, 0.0, 1.0) * (vocab - 1)).astype(np.int64) + 1, vocab - 1)
    mask = np.zeros((B, N), dtype=np.int64)
    if variant == 0:
        for r, n in enumerate(spec["lengths"]):
            mask[r, :n] = 1
    else:                                   # row 0: a prefix of another length; row 1: not a prefix at all
        mask[0, :max(1, N // 3)] = 1
        mask[1, 1::2] = 1
        mask[1, N - 1] = 1
    ids[mask == 0] = 0                      # the pad id
    return ids, mask


def state_dict(schema, seed=SEED):
    return {k: torch.from_numpy(fill(k, tuple(s), seed)) for k, s in schema}


def load_fixture():
    g = np.load(GOLDEN)
    out = {"bucket_row": g["bucket_row"]}
    for c in CASES:
        out[c] = dict(schema=[(k, tuple(s)) for k, s in json.loads(str(g[f"{c}.schema"]))], input_ids=g[f"{c}.input_ids"],
                      attention_mask=g[f"{c}.attention_mask"], out=g[f"{c}.out"], step=int(g[f"{c}.step"]))
    return out


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------
def bucket(rel, num_buckets=32, max_distance=128):
    """T5Attention._relative_position_bucket, bidirectional: torch float32 operations in Hugging Face's order"""
    nb = num_buckets // 2
    out = (rel > 0).to(torch.long) * nb
    rel = torch.abs(rel)
    exact = nb // 2
    large = exact + (torch.log(rel.float() / exact) / math.log(max_distance / exact) * (nb - exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return out + torch.where(rel < exact, rel, large)


def position_bias(rel_w, N):
    """[heads, N, N]: bias[h, i, j] = rel_w[bucket(j - i), h]"""
    pos = torch.arange(N)
    return rel_w[bucket(pos[None, :] - pos[:, None], rel_w.shape[0])].permute(2, 0, 1)


def rmsnorm(x, w, eps=EPS):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def attention(q, k, v, bias, mask, p_dtype=None):
    """q, k, v [B, H, N, d]; bias [H, N, N]; mask [B, N] (any pattern, != 0 keeps the key) -> [B, H, N, d].  No 1 / sqrt(d) scale;
    masked keys are excluded.  ``p_dtype``: P is rounded to it before P V (what the bf16 kernel does)."""
    s = q @ k.transpose(-1, -2) + bias[None]
    s = s.masked_fill((mask == 0)[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    if p_dtype is not None:
        p = p.to(p_dtype).to(q.dtype)
    return p @ v


def gate(u, gated):
    if not gated:
        return torch.relu(u)
    F = u.shape[-1] // 2
    return gelu_new(u[..., :F]) * u[..., F:]


def encoder(sd, input_ids, attention_mask, dtype=torch.float64, stream_dtype=None):
    """last_hidden_state [B, N, d_model] in ``stream_dtype`` (default: ``dtype``): the linears and the attention in ``dtype``, the residual
    stream and the norms in ``stream_dtype``"""
    stream_dtype = stream_dtype or dtype
    ids = torch.as_tensor(input_ids).to(sd["shared.weight"].device)
    mask = torch.as_tensor(attention_mask).to(ids.device)
    W = lambda k: sd[k].to(dtype)                                   # noqa: E731
    S = lambda k: sd[k].to(stream_dtype)                            # noqa: E731
    heads = sd[REL_BIAS].shape[1]
    B, N = ids.shape
    h = S("shared.weight")[ids]
    bias = position_bias(sd[REL_BIAS].float().cpu(), N).to(ids.device).to(dtype)
    i = 0
    while BLOCK.format(i, 0) + "SelfAttention.q.weight" in sd:
        a, f = BLOCK.format(i, 0), BLOCK.format(i, 1)
        n = rmsnorm(h, S(a + "layer_norm.weight")).to(dtype)
        split = lambda t: t.view(B, N, heads, -1).transpose(1, 2)     # noqa: E731
        q, k, v = (split(n @ W(a + f"SelfAttention.{x}.weight").t()) for x in "qkv")
        o = attention(q, k, v, bias, mask).transpose(1, 2).reshape(B, N, -1)
        h = h + (o @ W(a + "SelfAttention.o.weight").t()).to(stream_dtype)
        n = rmsnorm(h, S(f + "layer_norm.weight")).to(dtype)
        ff = f + "DenseReluDense."
        if ff + "wi_0.weight" in sd:
            u = gelu_new(n @ W(ff + "wi_0.weight").t()) * (n @ W(ff + "wi_1.weight").t())
        else:
            u = torch.relu(n @ W(ff + "wi.weight").t())
        h = h + (u @ W(ff + "wo.weight").t()).to(stream_dtype)
        i += 1
    return rmsnorm(h, S("encoder.final_layer_norm.weight"))


# ---- stubs of what stays the caller's -----------------------------------------------------------------------------------------------
class StubTokenizer:
    """stands in for ``AutoTokenizer``: one id per character (no SentencePiece model here), the reference's call signature"""

    def __init__(self, vocab=96):
        self.vocab, self.calls = vocab, 0

    def __call__(self, texts, truncation=True, max_length=128, padding="max_length", return_tensors="pt"):
        assert truncation is True and padding == "max_length" and return_tensors == "pt"
        self.calls += 1
        ids = torch.zeros((len(texts), max_length), dtype=torch.int64)
        mask = torch.zeros((len(texts), max_length), dtype=torch.int64)
        for r, t in enumerate(texts):
            toks = [2 + (ord(c) % (self.vocab - 2)) for c in t][:max_length - 1] + ([1] if t else [])      # 1: </s>
            ids[r, :len(toks)] = torch.tensor(toks, dtype=torch.int64)
            mask[r, :len(toks)] = 1
        return {"input_ids": ids, "attention_mask": mask}


def metrics(got, ref):
    """(relative L2, max-abs / max-ref) of ``got`` against ``ref``"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return (float(np.sqrt(((got - ref) ** 2).sum() / max((ref ** 2).sum(), 1e-300))), float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)))
