"""Dry run of the training path's host code: every library call it makes, recorded on the CPU.

    python tools/train_record.py --out record.json [--tree PATH] [--full] [--time N]
    python tools/train_record.py --compare A.json B.json
    python tools/train_record.py --write-fixture tests/golden/train_record.json

The library is replaced by a stand-in whose every function appends (name, arguments) to a list and returns 0 (1 for the ``*_fits``
queries), the runtime's device is the CPU and its stream 0: no host decision of the training path depends on a tensor's values, so the
operators (``conv1d_same`` / ``conv_transpose1d`` / ``linear`` / ``film_bank`` through autograd) and a whole
``GaussianDiffusion.training_loosses`` pass + ``backward()`` run without a GPU and leave their launch list behind: function name, every
scalar argument, every field of ``jen1_gemm_args`` / ``jen1_gemm_operand`` / ``jen1_bgemm_args`` (pointers as null / not null), and
``rt.stats`` after the case.  Two trees (``--tree``: a checkout of another commit) are compared launch by launch with ``--compare``;
tests/test_train_record_host.py compares this tree with the committed record.  The patches live here: the package is not changed for it.
"""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys
import time
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (kind, B, Ci, Co, L, k, stride, causal): causal False / True / a list = CausalRows over these flags.  linear: L rows per batch element
BF16_GRID = {
    "conv_2048": ("conv", 2, 128, 128, 2048, 3, 1, False),
    "conv_2047": ("conv", 2, 128, 128, 2047, 3, 1, False),
    "conv_2048_causal": ("conv", 2, 128, 128, 2048, 3, 1, True),
    "conv_2048_rows": ("conv", 3, 128, 128, 2048, 3, 1, [1, 0, 1]),
    "conv_8192_k5_s2_causal": ("conv", 2, 128, 256, 8192, 5, 2, True),
    "conv_ci257": ("conv", 2, 257, 128, 2048, 3, 1, False),
    "conv_co2": ("conv", 2, 128, 2, 2048, 3, 1, False),
    "convT_1024": ("convT", 2, 128, 128, 1024, 4, 2, False),
    "convT_512": ("convT", 2, 128, 128, 512, 4, 2, False),
    "convT_ci96": ("convT", 2, 96, 128, 1024, 4, 2, False),
    "linear_4096": ("linear", 1, 128, 128, 4096, 1, 1, False),
    "linear_16": ("linear", 1, 1024, 512, 16, 1, 1, False),
    "linear_2064_big": ("linear_nobias", 1, 1024, 1024, 2064, 1, 1, False),
    "film_bank": ("film_bank", 16, 512, 2048, 27, 1, 1, False),
    "conv_b16_l6": ("conv", 16, 128, 128, 6, 3, 1, False),
    "conv_l1": ("conv", 2, 64, 64, 1, 3, 1, False),
    "conv_odd": ("conv", 2, 16, 24, 37, 3, 1, False),
}
F32_GRID = {"conv_2048_f32": ("conv", 2, 128, 128, 2048, 3, 1, False)}
# (dtype, causal, what the stand-in answers to *_fits)
PASSES = {
    "pass_tiny_f32": ("f32", False, 1), "pass_tiny_f32_rows": ("f32", [1, 0], 1),
    "pass_tiny_bf16": ("bf16", False, 1), "pass_tiny_bf16_rows": ("bf16", [1, 0], 1),
    "pass_tiny_bf16_gemm_attn": ("bf16", False, 0),
}

class Recorder:
    """the stand-in for libjen1_hip.so"""

    def __init__(self, symbols):
        self.calls, self.fits, self.symbols = [], 1, symbols

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        types = self.symbols.get(name, (None, []))[1]

        def fn(*args):
            self.calls.append([name, [_plain(a, types[i] if i < len(types) else None) for i, a in enumerate(args)]])
            return self.fits if name.endswith("_fits") else 0
        self.__dict__[name] = fn
        return fn


def _plain(a, ctype=None):
    """pointer-free form of one argument"""
    if hasattr(a, "_obj"):                       # ctypes.byref(struct)
        a = a._obj
    if isinstance(a, C.Structure):
        return [_plain(getattr(a, f), t) for f, t in a._fields_]
    if ctype is C.c_void_p or (ctype is not None and hasattr(ctype, "contents")):
        return "ptr" if a else "null"
    if a is None:
        return "null"
    if isinstance(a, bool):
        return int(a)
    return a


@contextlib.contextmanager
def dry_run(tree):
    """the package of ``tree`` with the five patches in place -> (train module, recorder)"""
    sys.path.insert(0, os.path.join(tree, "jen-1-pytorch_amd"))
    import torch
    from jen1_amd import lib as L
    from jen1_amd import train as TR
    rec = Recorder({**L.SYMBOLS, **getattr(L, "T5_SYMBOLS", {})})
    init = TR.TrainRuntime.__init__

    def cpu_init(self, compute_dtype="bf16", device="cuda"):
        init(self, compute_dtype, "cuda")
        self.device = torch.device("cpu")
        self.stream = lambda: 0
    with mock.patch.object(L, "load", lambda: rec), mock.patch.object(TR.TrainRuntime, "__init__", cpu_init), \
            mock.patch.object(TR.TrainGraph, "_off_default_stream", lambda self, fn, *a, **k: fn(*a, **k)), \
            mock.patch.object(torch.cuda, "is_current_stream_capturing", lambda: False):
        yield TR, rec


def _case_result(rec, rt):
    return {"launches": rec.calls[:], "stats": {k: [v[0], float(v[1]), float(v[2])] for k, v in rt.stats.items()}}


def grid_case(TR, rec, case, dtype="bf16", **switches):
    """one operator through its autograd wrapper, forward then backward, on a fresh runtime with ``switches`` set"""
    import torch
    kind, B, ci, co, Lx, k, stride, causal = case
    rt = TR.TrainRuntime(dtype)
    rt.stats = {}
    for name, v in switches.items():
        assert hasattr(rt, name), name
        setattr(rt, name, v)
    par = lambda *shape: torch.nn.Parameter(torch.zeros(shape))
    rec.calls.clear()
    if kind == "film_bank":
        x = torch.zeros((B, ci), dtype=rt.tdtype, requires_grad=True)
        outs = [o for o, _ in TR.film_bank(rt, x, [par(co, ci) for _ in range(Lx)], [par(co) for _ in range(Lx)])]
        torch.autograd.backward(outs, [torch.zeros_like(o) for o in outs])
        return _case_result(rec, rt)
    x = torch.zeros((B, Lx, TR.pad8(ci)), dtype=rt.tdtype, requires_grad=True)
    if kind == "conv":
        c = TR.CausalRows(torch.tensor(causal)) if isinstance(causal, list) else causal
        y = TR.conv1d_same(rt, x, par(co, ci, k), par(co), stride, c)
    elif kind == "convT":
        y = TR.conv_transpose1d(rt, x, par(ci, co, k), par(co), stride, stride // 2 + stride % 2, stride % 2)
    else:
        y = TR.linear(rt, x, par(co, ci), None if kind == "linear_nobias" else par(co))
    y.backward(torch.zeros_like(y))
    return _case_result(rec, rt)


def reflect_case(TR, rec):
    """one forward with reflect padding, as the SEANet convolutions build it (encodec.py), bf16 at 4096 rows"""
    import torch
    rt = TR.TrainRuntime("bf16")
    rt.stats = {}
    B, ci, co, Lx, k = 2, 128, 128, 2048, 7
    x = torch.zeros((B, Lx, ci), dtype=rt.tdtype)
    wp = rt.packed(torch.zeros((co, ci, k)), "conv", x.dtype)
    rec.calls.clear()
    fwd = getattr(TR, "conv_forward", None) or TR._conv_forward
    fwd(rt, x, wp, torch.zeros(co), TR.ConvGeom("conv", k, 1, k // 2, Lx, Lx, ci, co, reflect=True))
    return _case_result(rec, rt)


def make_pass(TR, cfg_name, dtype, B, T):
    """model, graph and inputs of a training pass (the build is not part of a timed repetition)"""
    import torch
    from jen1_amd import config, synth
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.model import UNetCFG1d
    torch.manual_seed(0)
    cfg = config.full_model_config() if cfg_name == "full" else config.tiny_model_config()
    model = UNetCFG1d(**cfg, init_seed=None, compute_dtype=dtype, device="cpu")
    model.train()
    graph = TR.TrainGraph(model, model.spec, dtype)
    betas, _ = get_beta_schedule("linear", 1000)
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cpu", cfg_dropout_proba=0.2,
                           embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    x0 = torch.from_numpy(synth.latents(B, T, key="clip"))
    cond = {k: None if v is None else torch.from_numpy(v) for k, v in synth.conditioning(B, T, "music_inpaint").items()}
    return model, graph, gd, x0, torch.arange(B) * 7 + 3, cond


def run_pass(rec, made, causal):
    import torch
    model, graph, gd, x0, t, cond = made
    for p in model.parameters():
        p.grad = None
    graph.rt.stats = {}
    rec.calls.clear()
    loss = gd.training_loosses(graph, x0, t, cond, causal=torch.tensor(causal) if isinstance(causal, list) else causal)
    n_fwd = len(rec.calls)
    (loss * 0.1).backward()
    return n_fwd


def pass_case(TR, rec, cfg_name, dtype, causal, fits, B, T):
    rec.fits = fits
    try:
        made = make_pass(TR, cfg_name, dtype, B, T)
        n_fwd = run_pass(rec, made, causal)
        out = dict(_case_result(rec, made[1].rt), forward_launches=n_fwd)
        made[1].rt.stats = None
        rec.calls.clear()
        made[1].rt.invalidate()
        made[1].rt.refresh_all()
        out["refresh"] = rec.calls[:]
        return out
    finally:
        rec.fits = 1


def build_record(tree=ROOT, full=False, only=None):
    rec_out = {}
    want = lambda name: only is None or name in only
    with dry_run(tree) as (TR, rec):
        for name, case in BF16_GRID.items():
            if want(name):
                rec_out[name] = grid_case(TR, rec, case)
                rec_out[name + "/unpaired"] = grid_case(TR, rec, case, pair_grads=False)
        for name, case in F32_GRID.items():
            if want(name):
                rec_out[name] = grid_case(TR, rec, case, "f32")
                rec_out[name + "/unpaired"] = grid_case(TR, rec, case, "f32", pair_grads=False)
        if want("conv_reflect_forward"):
            rec_out["conv_reflect_forward"] = reflect_case(TR, rec)
        for name, (dtype, causal, fits) in PASSES.items():
            if want(name):
                rec_out[name] = pass_case(TR, rec, "tiny", dtype, causal, fits, 2, 96)
        if full:
            rec_out["pass_full_bf16"] = pass_case(TR, rec, "full", "bf16", False, 1, 2, 1500)
    return json.loads(json.dumps(rec_out))


def time_full(tree, reps):
    """host cost of the eager full-size pass, forward + backward, model build excluded: seconds per repetition"""
    with dry_run(tree) as (TR, rec):
        made = make_pass(TR, "full", "bf16", 2, 1500)
        run_pass(rec, made, False)
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run_pass(rec, made, False)
            out.append(round(time.perf_counter() - t0, 3))
    return out


def first_difference(a, b):
    """None when two records agree; the refreshes of ``refresh_all`` compare as a set (their order is free)"""
    if list(a) != list(b):
        return f"cases differ: {sorted(set(a) ^ set(b))}"
    for name in a:
        ca, cb = a[name], b[name]
        for i, (x, y) in enumerate(zip(ca["launches"], cb["launches"])):
            if x != y:
                return f"{name}: launch {i}: {json.dumps(x)} against {json.dumps(y)}"
        if len(ca["launches"]) != len(cb["launches"]):
            return f"{name}: {len(ca['launches'])} launches against {len(cb['launches'])}"
        if ca["stats"] != cb["stats"]:
            return f"{name}: stats {ca['stats']} against {cb['stats']}"
        if ca.get("forward_launches") != cb.get("forward_launches"):
            return f"{name}: {ca.get('forward_launches')} forward launches against {cb.get('forward_launches')}"
        ra, rb = (sorted(json.dumps(x) for x in c.get("refresh", [])) for c in (ca, cb))
        if ra != rb:
            return f"{name}: refresh_all: {[x for x in ra if x not in rb][:1]} against {[x for x in rb if x not in ra][:1]}"
    return None


def write_fixture(rec, path):
    """each distinct launch once (``table``, one per line), the cases as index sequences into it"""
    table, index = [], {}

    def ref(entry):
        key = json.dumps(entry)
        if key not in index:
            index[key] = len(table)
            table.append(entry)
        return index[key]
    cases = {name: {k: ([ref(e) for e in v] if k in ("launches", "refresh") else v) for k, v in c.items()} for name, c in rec.items()}
    with open(path, "w") as fh:
        fh.write('{\n "table": [\n' + ",\n".join("  " + json.dumps(e, separators=(",", ":")) for e in table) + '\n ],\n "cases": {\n')
        fh.write(",\n".join(f"  {json.dumps(n)}: {json.dumps(c, separators=(',', ':'))}" for n, c in cases.items()))
        fh.write("\n }\n}\n")


def load_fixture(path):
    with open(path) as fh:
        fx = json.load(fh)
    return {name: {k: ([fx["table"][i] for i in v] if k in ("launches", "refresh") else v) for k, v in c.items()} for name, c in fx["cases"].items()}


def load(path):
    with open(path) as fh:
        head = json.load(fh)
    return load_fixture(path) if "table" in head else head


def summary(rec):
    for name, c in rec.items():
        names = [e[0] for e in c["launches"]]
        big = {n: names.count(n) for n in ("jen1_big_gemm_conv", "jen1_big_gemm_tn_conv", "jen1_big_gemm", "jen1_big_gemm_tn_store")}
        fwd = f", {c['forward_launches']} forward" if "forward_launches" in c else ""
        print(f"{name}: {len(names)} launches{fwd}; " + " / ".join(str(v) for v in big.values()) + " of " + ", ".join(n[5:] for n in big))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package runs (default: this one)")
    ap.add_argument("--out")
    ap.add_argument("--write-fixture")
    ap.add_argument("--full", action="store_true", help="also the full configuration, bf16, B = 2, T = 1500")
    ap.add_argument("--time", type=int, default=0, help="time the full-size pass N times instead")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        a, b = (load(p) for p in args.compare)
        d = first_difference(a, b)
        print(f"{len(a)} cases, {sum(len(c['launches']) for c in a.values())} launches: " + ("no difference" if d is None else "first difference: " + d))
        return 1 if d else 0
    if args.time:
        print(json.dumps({"full_pass_host_s": time_full(args.tree, args.time)}))
        return 0
    rec = build_record(args.tree, args.full)
    summary(rec)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rec, fh)
    if args.write_fixture:
        write_fixture({k: v for k, v in rec.items() if k != "pass_full_bf16"}, args.write_fixture)
    return 0


if __name__ == "__main__":
    sys.exit(main())
