#!/usr/bin/env python3
"""What the host builder (jen1_amd/engine.py) decides, written down without a pointer in it: for a fixed list of plans -- one per
execution form, at the smallest shape the suite uses for it -- the launch ops (kind, label, traffic / work accounting), the phase lists
of the persistent programs and the counts; after one seeded run also the error word and the SHA-256 of the network's output and of
every activation.  Two engines that record the same thing build the same launches; tests/test_gpu_plan_record.py keeps the record
without the hashes (tests/golden/plan_record.json) as a fixture.

    python tools/plan_record.py --out record.json            # build, run, hash (GPU box)
    python tools/plan_record.py --no-run --out golden.json   # no run, no hashes, the fixture's compact form (write_fixture)
    python tools/plan_record.py --compare A.json A2.json B.json
        A, A2: two runs of the engine before a change, B: the engine after it.  Hashes are compared for the cases whose hashes agree
        between A and A2 (the others use float atomics somewhere: compared on the record alone); an empty label of A matches any label.
"""
import argparse
import contextlib
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jen-1-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

F_CTX = 24          # context_features of the tiny configuration's per-sample case (tests/test_gpu_global_cond.py)

# name -> model (configuration, dtype), shape, Plan keywords, engine attributes held while the plan is built, hashes after a run
_full = dict(cfg="full", dtype="bf16", B=2, T=1500, nrep=1, causal=False)
CASES = {
    "bf16": dict(_full),
    "bf16_pair_causal": dict(_full, nrep=2, causal=True),
    "f32": dict(_full, dtype="f32"),
    "fp8": dict(_full, dtype="fp8"),
    "launch_fixed_order": dict(_full, deep=False, deterministic=True),
    "launch": dict(_full, deep=False, hashes=False),                       # float atomics: the record alone
    "no_long": dict(_full, eng=dict(use_long=False)),
    "tile_phases": dict(_full, eng=dict(use_tile_phases=True)),            # JEN1_TILE_PHASES=1
    "no_fold_up": dict(_full, eng=dict(fold_up=frozenset())),              # JEN1_FOLD_UP=0
    "table_nt4": dict(_full, n_t=4),
    # (launch-per-layer levels: fixed-order statistics, so that the hashes mean something)
    "tiny_per_sample": dict(cfg="tiny_features", dtype="f32", B=3, T=96, nrep=2, causal=False, n_t=4, per_sample=True, deterministic=True),
}
OP_FIELDS = ("kind", "label", "w_bytes", "act_bytes", "flops", "bytes")


def make_model(cfg: str, dtype: str):
    from jen1_amd.config import full_model_config, tiny_model_config
    from jen1_amd.model import UNetCFG1d
    kw = full_model_config() if cfg == "full" else dict(tiny_model_config(), context_features=F_CTX)
    return UNetCFG1d(**kw, init_seed=1234, compute_dtype=dtype, device="cuda")


@contextlib.contextmanager
def engine_attrs(eng, attrs):
    old = {k: getattr(eng, k) for k in attrs}
    for k, v in attrs.items():
        setattr(eng, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(eng, k, v)


def build_plan(model, case):
    """built directly: the engine's plan cache is keyed without the knobs"""
    from jen1_amd.engine import Plan
    eng = model.engine()
    with engine_attrs(eng, case.get("eng", {})):
        return Plan(eng, case["B"], case["T"], case["nrep"], case["causal"], case.get("n_t"), deep=case.get("deep", True),
                    deterministic=case.get("deterministic", False), per_sample=case.get("per_sample", False))


def op_record(op):
    return [getattr(op, "kind", ""), getattr(op, "label", "")] + [getattr(op, f, 0) for f in OP_FIELDS[2:]]


def plan_record(plan) -> dict:
    return {
        "ops": [op_record(op) for op in plan.ops],
        "time_ops": [op_record(op) for op in plan.time_ops],
        "ctx_ops": [op_record(op) for op in plan.ctx_ops],
        "progs": [dict(kinds=list(p.kinds), labels=list(p.labels), lds=int(p.lds), nwg=int(p.nwg), poison_rows=int(p.poison_tab.shape[0]),
                       poison_bytes=int(p.poison_bytes)) for p in plan.progs],
        "deep_level": plan.deep_level, "long_levels": plan.long_levels, "folded_levels": list(plan.folded_levels),
        "deep_errors": list(plan.deep_errors), "long_errors": list(plan.long_errors), "tile_errors": list(plan.tile_errors),
        "fold_errors": list(plan.fold_errors), "n_launch": plan.n_launch, "n_acts": len(plan.acts), "arena_words": int(plan._arena_used),
    }


def _sha(t) -> str:
    import torch
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def run_record(model, plan, case) -> dict:
    """one seeded run (synth.latents / synth.conditioning, the timesteps of tests/test_gpu_long.py) -> error word and hashes; the
    descriptor images hold device addresses and go under a key of their own (equal only when two processes allocate identically)"""
    import numpy as np
    import torch
    from jen1_amd import synth
    from jen1_amd.init_fill import fill_normal
    B, T = case["B"], case["T"]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x, cond = synth.latents(B, T), synth.conditioning(B, T, "music_cont" if case["causal"] else "text_guided")
    times = lambda n: dev(np.array([(131 * i + 7) % 1000 for i in range(n)], dtype=np.int64))
    feats = dev(fill_normal("synth.features", (B, F_CTX), 5).astype(np.float32)) if plan.has_features else None
    s = torch.cuda.current_stream().cuda_stream
    model._prepare(plan, dev(x), times(B), dev(cond["cross_attn_cond"]), dev(cond["cross_attn_masks"]), [dev(cond["input_concat_cond"])], None,
                   features=feats)
    if plan.table_mode:
        plan.set_times(times(plan.n_t))
        plan.run_time(s)
        plan.step_idx.zero_()
    plan.run(s)
    torch.cuda.synchronize()
    out = {"take_error": int(plan.take_error()), "addresses": {"dev": [_sha(p.dev) for p in plan.progs]}}
    if case.get("hashes", True):
        out["net_out"] = _sha(plan.net_out.t)
        out["acts"] = [_sha(a.t) for a in plan.acts]
    return out


def check_forms(rec: dict):
    """every case holds the form it is there for, and each back end of ``conv`` appears somewhere: else the shapes were chosen wrongly"""
    labels = lambda c: [o[1] for o in rec[c]["ops"] + rec[c]["time_ops"]]
    kinds = lambda c: [o[0] for o in rec[c]["ops"]]
    pk = lambda c: [p["kinds"] for p in rec[c]["progs"]]
    for c in ("bf16", "bf16_pair_causal", "f32", "fp8", "no_fold_up", "table_nt4"):
        k = pk(c)
        assert len(k) == 3 and k[0][0] == "long" and k[-1][0] == "long" and "gemm" in k[1] and "attn" in k[1], (c, [x[:2] for x in k])
        assert rec[c]["long_levels"] >= 1 and not rec[c]["long_errors"], (c, rec[c]["long_errors"])
    assert sorted(rec["bf16"]["folded_levels"]) == [3, 4, 5, 6, 7, 8] and rec["no_fold_up"]["folded_levels"] == []
    assert len(rec["no_fold_up"]["progs"][1]["kinds"]) == len(rec["bf16"]["progs"][1]["kinds"]) + 6
    assert rec["no_long"]["long_levels"] == 0 and all(k[0] != "long" for k in pk("no_long")) and any("gemm" in k for k in pk("no_long"))
    assert sum(k.count("tile") for k in pk("tile_phases")) >= 20 and not rec["tile_phases"]["tile_errors"], rec["tile_phases"]["tile_errors"]
    for c in ("launch", "launch_fixed_order"):
        assert rec[c]["progs"] == [] and rec[c]["deep_level"] is None
        assert any(" direct=1" in l for l in labels(c)) and any(l.startswith("conv[") and " sk=1 " not in l for l in labels(c)), c
        assert "norm_apply" in kinds(c), c
    assert kinds("launch_fixed_order").count("stats") > 0 and kinds("launch").count("stats") == 0
    assert "film_select" in kinds("tiny_per_sample") and rec["tiny_per_sample"]["long_levels"] == 0


def structure(rec: dict) -> dict:
    """the record without what a run adds"""
    return {c: {k: v for k, v in r.items() if k != "run"} for c, r in rec.items()}


def digest(obj) -> str:
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()


def write_fixture(rec: dict, path: str):
    """the record without hashes in the fixture's form: most ops and phases repeat within and across the plans, so every distinct one
    -- an op's (kind, label, w_bytes, act_bytes, flops, bytes), a phase's (kind, label) -- stands once in ``table``, one per line, and
    the plans hold sequences of indices into it (a changed heuristic shows as a changed table line, a changed order as changed indices)"""
    table, index = [], {}

    def ref(entry) -> int:
        key = json.dumps(entry)
        if key not in index:
            index[key] = len(table)
            table.append(entry)
        return index[key]
    plans = {}
    for c, r in structure(rec).items():
        p = dict(r, **{k: [ref(o) for o in r[k]] for k in ("ops", "time_ops", "ctx_ops")})
        p["progs"] = [dict({k: v for k, v in q.items() if k not in ("kinds", "labels")}, phases=[ref([kd, lb]) for kd, lb in zip(q["kinds"], q["labels"])])
                      for q in r["progs"]]
        plans[c] = p
    with open(path, "w") as fh:
        fh.write('{\n "table": [\n' + ",\n".join("  " + json.dumps(e) for e in table) + '\n ],\n "plans": {\n')
        fh.write(",\n".join(f"  {json.dumps(c)}: {{\n" + ",\n".join(f"   {json.dumps(k)}: {json.dumps(v)}" for k, v in p.items()) + "\n  }" for c, p in plans.items()))
        fh.write("\n }\n}\n")


def load_fixture(path: str) -> dict:
    """``write_fixture`` undone: the record as ``plan_record`` gives it"""
    with open(path) as fh:
        fx = json.load(fh)
    table, rec = fx["table"], {}
    for c, p in fx["plans"].items():
        r = dict(p, **{k: [table[i] for i in p[k]] for k in ("ops", "time_ops", "ctx_ops")})
        r["progs"] = [dict({k: v for k, v in q.items() if k != "phases"}, kinds=[table[i][0] for i in q["phases"]], labels=[table[i][1] for i in q["phases"]])
                      for q in p["progs"]]
        rec[c] = r
    return rec


def diff_structure(a, b, path=""):
    """differences of two structures; an empty label of ``a`` (an op that had none) matches any label of ``b``"""
    if isinstance(a, dict) and isinstance(b, dict):
        return [d for k in sorted(set(a) | set(b)) for d in (diff_structure(a[k], b[k], f"{path}/{k}") if k in a and k in b else [f"{path}/{k}: only in one"])]
    if isinstance(a, list) and isinstance(b, list):
        if len(a) != len(b):
            return [f"{path}: {len(a)} entries against {len(b)}"]
        is_op = len(a) == len(OP_FIELDS) and isinstance(a[0], str) and isinstance(a[1], str) and path.split("/")[-2:-1] in (["ops"], ["time_ops"], ["ctx_ops"])
        if is_op and a[1] == "":
            a = [a[0], b[1]] + a[2:]
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in diff_structure(x, y, f"{path}/{i}")]
    return [] if a == b else [f"{path}: {a!r} against {b!r}"]


def compare(pa: str, pa2: str, pb: str) -> int:
    A, A2, Bn = (json.load(open(p)) for p in (pa, pa2, pb))
    print(f"record digest (without hashes): before {digest(structure(A))}, before again {digest(structure(A2))}, after {digest(structure(Bn))}")
    bad = diff_structure(structure(A), structure(A2), "before-vs-before")
    diffs = diff_structure(structure(A), structure(Bn))
    new_labels = sum(1 for c in A for k in ("ops", "time_ops", "ctx_ops") for x, y in zip(A[c][k], Bn[c][k]) if x[1] == "" and y[1] != "") if not diffs else 0
    print(f"records: {len(diffs)} differences over {len(A)} plans ({new_labels} ops that had no label were given one)")
    hashed = lambda r: {k: r["run"].get(k) for k in ("net_out", "acts")} if "net_out" in r.get("run", {}) else None
    stable = [c for c in A if hashed(A[c]) is not None and hashed(A[c]) == hashed(A2[c])]
    unstable = [c for c in A if hashed(A[c]) is not None and c not in stable]
    print(f"hashes reproducible between the two runs before the change (compared): {', '.join(stable) or '-'}")
    print(f"hashes that differ between the two runs before the change (record alone): {', '.join(unstable) or '-'}")
    print(f"no hashes by construction (record alone): {', '.join(c for c in A if hashed(A[c]) is None) or '-'}")
    for c in stable:
        hb = hashed(Bn[c])
        same = hb == hashed(A[c])
        n = len(A[c]["run"]["acts"])
        print(f"  {c}: net_out {A[c]['run']['net_out'][:16]} + {n} activations {digest(A[c]['run']['acts'])[:16]}: {'equal' if same else 'DIFFERENT'} after the change")
        if not same:
            diffs.append(f"{c}: hashes differ")
    for c in A:
        if A[c].get("run", {}).get("take_error", 0) or Bn[c].get("run", {}).get("take_error", 0):
            diffs.append(f"{c}: error word {A[c]['run']['take_error']} / {Bn[c]['run']['take_error']}")
    dev_same = [c for c in A if A[c]["progs"] and A[c]["run"]["addresses"] == Bn[c]["run"]["addresses"]]
    print(f"descriptor images (hold device addresses; a bonus, equal only when both processes allocate identically): byte-equal in "
          f"{len(dev_same)} of {sum(1 for c in A if A[c]['progs'])} plans with programs ({', '.join(dev_same) or '-'})")
    for d in (bad + diffs)[:40]:
        print("  DIFFERENCE", d)
    print("verdict:", "EQUAL" if not (bad or diffs) else "NOT EQUAL")
    return 0 if not (bad or diffs) else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="write the record here (JSON)")
    ap.add_argument("--no-run", action="store_true", help="build and record only: no run, no hashes; --out is then written in the fixture's form")
    ap.add_argument("--cases", help="comma list of case names (default: all)")
    ap.add_argument("--compare", nargs=3, metavar=("A", "A2", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    names = args.cases.split(",") if args.cases else list(CASES)
    models, rec = {}, {}
    for name in names:
        case = CASES[name]
        key = (case["cfg"], case["dtype"])
        if key not in models:
            models[key] = make_model(*key)
        plan = build_plan(models[key], case)
        rec[name] = plan_record(plan)
        if not args.no_run:
            rec[name]["run"] = run_record(models[key], plan, case)
        print(f"{name}: {len(plan.ops)} ops, {[len(p) for p in plan.progs]} phases, {plan.n_launch} launches"
              + ("" if args.no_run else f", error word {rec[name]['run']['take_error']}"), flush=True)
    if args.out and args.no_run:
        write_fixture(rec, args.out)
    elif args.out:
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    if not args.cases:
        check_forms(rec)
    print(f"record digest (without hashes): {digest(structure(rec))}")


if __name__ == "__main__":
    main()
