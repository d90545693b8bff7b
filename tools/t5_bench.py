"""Times the captured T5 encoder of jen1_amd/t5.py at flan-t5-large geometry (24 layers, 1024 / 16 x 64 / 2816, N = 128) with filled
weights, B = 8 (the bench workload's batch) and B = 3 (the conditioner calls of one trainer micro-batch), in f32 and bf16, against what a
caller has without it: the same stack on stock torch operators on the same GPU (tests/t5_common.py's restatement in float32 / bfloat16
with a float32 residual stream) and, where ``transformers`` imports, ``T5EncoderModel`` itself.

Times are device events around REPS back-to-back passes after WARM warm-up passes, alternating the three paths ROUNDS times; the median
round is reported with the spread.  ``call`` is ``T5EncoderHIP.__call__`` as a user makes it (input copies, replay, output copy, the
id-range flag read back); ``replay`` is the graph alone.  Reported, not gated: writes one line per (mode, B) and needs a GPU.

    python tools/t5_bench.py [--layers 24] [--out profiles/t5_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jen-1-pytorch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import t5_common as TC  # noqa: E402

WARM, REPS, ROUNDS = 3, 10, 5


def timed(fn) -> float:
    """ms per pass of ``fn`` over REPS passes, by device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--vocab", type=int, default=32128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("t5_bench needs a GPU: there is no CPU timing of this path")
    from jen1_amd.t5 import T5EncoderHIP
    geo = dict(vocab=args.vocab, d_model=1024, heads=16, d_kv=64, d_ff=2816, layers=args.layers, gated=True)
    sd = TC.state_dict(TC.schema_of(**geo))
    sd_gpu = {k: v.cuda() for k, v in sd.items()}
    hf = None
    try:
        from transformers import T5Config, T5EncoderModel
        cfg = T5Config(vocab_size=geo["vocab"], d_model=1024, d_kv=64, d_ff=2816, num_layers=args.layers, num_heads=16, dropout_rate=0.0,
                       feed_forward_proj="gated-gelu")
        hf = T5EncoderModel(cfg).eval()
        hf.load_state_dict({**sd, "encoder.embed_tokens.weight": sd["shared.weight"]}, strict=False)
    except ImportError:
        pass
    lines = [f"# T5 encoder, flan-t5-large geometry, {args.layers} layers, N = 128; ms per pass, median of {ROUNDS} rounds of {REPS} (min .. max)"]
    N = 128
    for mode, tdt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        enc = T5EncoderHIP.from_state_dict(sd, compute_dtype=mode)
        hf_m = None if hf is None else hf.to("cuda", tdt)
        sd_t = {k: v.to(tdt) for k, v in sd_gpu.items()}
        for B in (8, 3):
            ids = torch.randint(1, geo["vocab"], (B, N), generator=torch.Generator().manual_seed(B)).cuda()
            mask = torch.ones((B, N), dtype=torch.int64, device="cuda")
            mask[:, 40:] = 0                                           # a prompt of 40 tokens padded to max_length
            mask[0] = 1
            paths = {"hip call": lambda: enc(ids, mask), "hip replay": lambda: enc._bufs[(B, N)].graph.replay(),
                     "torch ops": lambda: TC.encoder(sd_t, ids, mask, dtype=tdt, stream_dtype=torch.float32)}
            if hf_m is not None:
                paths["transformers"] = lambda: hf_m(input_ids=ids, attention_mask=mask.bool())["last_hidden_state"]
            with torch.no_grad():
                y = enc(ids, mask)
                ref = TC.encoder(sd_t, ids, mask, dtype=tdt, stream_dtype=torch.float32)
                l2, mx = TC.metrics(y.cpu().numpy(), ref.float().cpu().numpy())
                for fn in paths.values():
                    for _ in range(WARM):
                        fn()
                torch.cuda.synchronize()
                times = {k: [] for k in paths}
                for _ in range(ROUNDS):
                    for k, fn in paths.items():
                        times[k].append(timed(fn))
            parts = [f"{k} {statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})" for k, v in times.items()]
            lines.append(f"{mode} B={B}: launches {enc.launches}; " + "; ".join(parts) + f"; hip vs torch ops of the same dtype: relative L2 {l2:.2e}, max-abs/max-ref {mx:.2e}")
            print(lines[-1], flush=True)
        del enc, hf_m, sd_t
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
