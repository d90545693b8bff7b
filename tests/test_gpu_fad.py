"""-m gpu: the Frechet Audio Distance on the HIP kernels (csrc/vggish.hip, jen1_amd/fad.py) against the checkers of tests/fad_common.py.

Where a tolerance is not fixed by construction it follows the project's rule: for the same input the test measures what the float32 CPU
chain (numpy for the front end, ``torch.nn`` for the network) loses against float64, and the kernel is allowed 8x that.  ``jen1_conv3x3``
has an elementwise bound instead: |err| <= 1e-6 (|W| * |x| + |b|), about three times the largest per-product-sum figure known for the
float32 matrix instruction (3.5e-7 at K = 4096; the largest K here is 4608).  Every test prints the figures it measured;
profiles/fad_parity.txt records them."""
import functools

import numpy as np
import pytest
import torch

import fad_common as O

pytestmark = pytest.mark.gpu

GUARD = 64                                          # floats of NaN on either side of a tensor under test (a multiple of 4: 16-byte alignment)
CONV_BOUND = 1e-6
CONV_CASES = [                                      # (N, H, W, Cin, Cout, pool)
    (1, 2, 2, 16, 16, True),                        # every tap of every position touches a border
    (3, 12, 8, 64, 128, True),                      # a deep layer's geometry; adjacent examples must not leak into each other
    (2, 6, 4, 48, 80, False),                       # channel counts that fill no whole tile
    (1, 24, 16, 128, 256, False),                   # a middle layer's geometry
    (2, 48, 32, 16, 32, True),                      # the largest plane
    (2, 3, 5, 32, 16, False),                       # odd H and W
    (5, 6, 4, 512, 512, False),                     # the longest K chain, several channel tiles
]


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd import fad
    return fad


@pytest.fixture(scope="module")
def L():
    from jen1_amd import lib
    lib.build()
    lib.load()
    return lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(shape):
    """(the whole buffer, the tensor inside it): NaN everywhere"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_intact(buf) -> bool:
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


# ------------------------------------------------------------------ front end
def front_gate(x_rows, got, what):
    """got [N, 96, 64] against the float64 restatement of the rows (lists of 16 kHz signals), gate 8x the float32 restatement's error"""
    want = np.concatenate([O.examples(x) for x in x_rows])
    f32 = np.concatenate([O.examples(x, np.float32) for x in x_rows])
    yard, err = O.rel_max(f32, want), O.rel_max(got, want)
    print(f"{what}: {want.shape[0]} examples, kernel {err:.3e}, float32 numpy {yard:.3e}, gate {O.TOL_FACTOR * yard:.3e}")
    assert got.shape == want.shape
    assert np.isfinite(got).all()
    assert err <= O.TOL_FACTOR * yard


def test_front_end_at_16k_rows_of_three_lengths(F):
    lengths = [15600, 30959, 30960]
    x = np.zeros((3, 1, 30960), dtype=np.float32)
    rows = [O.mix(n, 7 + i) for i, n in enumerate(lengths)]
    for i, r in enumerate(rows):
        x[i, 0, :len(r)] = r
    ex, counts = F.vggish_examples(torch.from_numpy(x).cuda(), 16000, lengths=lengths)
    assert counts == [1, 1, 2] and tuple(ex.shape) == (4, 96, 64)
    front_gate(rows, ex.cpu().numpy(), "front end, 16 kHz, lengths 15600 / 30959 / 30960")
    # without lengths every row counts in full: the padded first row gives the examples of the padded signal
    ex2, counts2 = F.vggish_examples(torch.from_numpy(x).cuda(), 16000)
    assert counts2 == [2, 2, 2] and torch.equal(ex2[0], ex[0]) and torch.equal(ex2[4:], ex[2:])


def test_front_end_too_short_gives_no_example(F):
    ex, counts = F.vggish_examples(torch.from_numpy(O.mix(15599, 3)).cuda().view(1, 1, -1), 16000)
    assert counts == [0] and tuple(ex.shape) == (0, 96, 64)
    ex, counts = F.vggish_examples(torch.zeros(2, 1, 100, device="cuda"), 16000)
    assert counts == [0, 0] and tuple(ex.shape) == (0, 96, 64)


def test_front_end_from_48k_stereo(F):
    from jen1_amd.audio import convert_audio
    n = 48000 + 1234
    wav = torch.from_numpy(np.stack([np.stack([O.mix(n, 20 + 2 * b, 48000), O.mix(n, 21 + 2 * b, 48000)]) for b in range(2)])).cuda()
    x16 = convert_audio(wav, 48000, 16000, 1, device="cuda")
    ex, counts = F.vggish_examples(wav, 48000)
    assert counts == [O.count(int(x16.shape[-1]))] * 2 == [1, 1]
    front_gate([r for r in x16.reshape(2, -1).cpu().numpy()], ex.cpu().numpy(), "front end, 48 kHz stereo through convert_audio")


# ------------------------------------------------------------------ jen1_conv3x3
@functools.lru_cache(maxsize=None)
def conv_data(case):
    N, H, W, cin, cout, pool = case
    rng = np.random.default_rng([11, N, H, W, cin, cout])
    x = rng.standard_normal((N, H, W, cin)).astype(np.float32)
    w = (rng.uniform(-1, 1, (cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    b = rng.uniform(-0.2, 0.2, cout).astype(np.float32)
    want, mag = O.conv_ref(x, w, b, pool)
    return x, w, b, want, mag


def run_conv(F, L, x, w, b, pool):
    """x [N, H, W, Cin] numpy -> (y numpy, guards intact): input and output inside NaN-filled buffers"""
    N, H, W, cin = x.shape
    cout = w.shape[0]
    xb, xt = guarded(x.shape)
    xt.copy_(torch.from_numpy(x))
    yb, yt = guarded((N, H // 2 if pool else H, W // 2 if pool else W, cout))
    packed = F.pack_conv3x3(torch.from_numpy(w)).cuda()
    assert packed.numel() == L.load().jen1_conv3x3_packed_floats(cin, cout)
    bt = torch.from_numpy(b).cuda()
    L.check(L.load().jen1_conv3x3(xt.data_ptr(), packed.data_ptr(), bt.data_ptr(), yt.data_ptr(), N, H, W, cin, cout, int(pool), stream()),
            "jen1_conv3x3")
    torch.cuda.synchronize()
    return yt.cpu().numpy(), guards_intact(yb) and guards_intact(xb)


@pytest.mark.parametrize("case", CONV_CASES, ids=["-".join(str(int(v)) for v in c) for c in CONV_CASES])
def test_conv3x3_against_float64(F, L, case):
    N, H, W, cin, cout, pool = case
    x, w, b, want, mag = conv_data(case)
    got, intact = run_conv(F, L, x, w, b, pool)
    assert intact, "a guard region was written"
    assert np.isfinite(got).all(), "a padded tap was read"
    ratio = float((np.abs(got.astype(np.float64) - want) / mag).max())
    print(f"jen1_conv3x3 {case}: K = {9 * cin}, worst |err| / (|W| * |x| + |b|) = {ratio:.3e} (bound {CONV_BOUND:.0e}), "
          f"max-abs / max = {O.rel_max(got, want):.3e}")
    assert ratio <= CONV_BOUND
    for i in range(N):                               # an example alone: the same bits as its slice of the batch
        alone, ok = run_conv(F, L, x[i:i + 1], w, b, pool)
        assert ok and np.array_equal(alone[0], got[i]), i


# ------------------------------------------------------------------ first layer
@pytest.mark.parametrize("cout", [16, 64])
def test_first_layer_from_a_mel_buffer(F, L, cout):
    rows, frames = 2, 96 + 7
    rng = np.random.default_rng([5, cout])
    mel = np.exp(2.5 * rng.standard_normal((rows, 64, frames)) - 2.0).astype(np.float32)
    mel[0, :, 10:14] = 0.0                           # silent frames: log(0.01)
    w = (rng.uniform(-1, 1, (cout, 1, 3, 3)) / 3.0).astype(np.float32)
    b = rng.uniform(-0.2, 0.2, cout).astype(np.float32)
    Fn = torch.nn.functional

    def ref(dtype):
        ex = torch.log(torch.from_numpy(mel[:, :, :96]).to(dtype) + 0.01).permute(0, 2, 1)[:, None]
        y = Fn.max_pool2d(Fn.relu(Fn.conv2d(ex, torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype), padding=1)), 2, 2)
        return y.permute(0, 2, 3, 1).numpy()
    want, f32 = ref(torch.float64), ref(torch.float32)
    mb, mt = guarded(mel.shape)
    mt.copy_(torch.from_numpy(mel))
    yb, yt = guarded((2, 48, 32, cout))
    wt = torch.from_numpy(w).reshape(cout, 9).t().contiguous().cuda()
    bt = torch.from_numpy(b).cuda()
    counts = (L.c_int * rows)(1, 1)
    L.check(L.load().jen1_vggish_conv1(mt.data_ptr(), counts, rows, frames, 0, 0, 2, wt.data_ptr(), bt.data_ptr(), yt.data_ptr(), cout, stream()),
            "jen1_vggish_conv1")
    torch.cuda.synchronize()
    got = yt.cpu().numpy()
    yard, err = O.rel_max(f32, want), O.rel_max(got, want)
    print(f"first layer, Cout {cout}: kernel {err:.3e}, float32 torch {yard:.3e}, gate {O.TOL_FACTOR * yard:.3e}")
    assert guards_intact(yb) and guards_intact(mb) and np.isfinite(got).all()
    assert err <= O.TOL_FACTOR * yard
    # the second example alone (first = 1, n = 1): the same bits
    y1b, y1 = guarded((1, 48, 32, cout))
    L.check(L.load().jen1_vggish_conv1(mt.data_ptr(), counts, rows, frames, 0, 1, 1, wt.data_ptr(), bt.data_ptr(), y1.data_ptr(), cout, stream()),
            "jen1_vggish_conv1")
    assert guards_intact(y1b) and torch.equal(y1[0], yt[1])


# ------------------------------------------------------------------ whole network
def net_examples(n, seed):
    rng = np.random.default_rng([9, n, seed])
    return np.maximum(1.8 * rng.standard_normal((n, 96, 64)) - 1.0, np.log(0.01)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def net_data(kind):
    widths, n = (O.NARROW, 3) if kind == "narrow" else (O.FULL, 2)
    model = O.VGGishModel(**widths, seed=21)
    ex = net_examples(n, 1)
    return model, ex, O.run_model(model, ex, torch.float64), O.run_model(model, ex, torch.float32)


@pytest.mark.parametrize("final_relu", [False, True])
@pytest.mark.parametrize("kind", ["narrow", "full"])
def test_whole_network(F, kind, final_relu):
    model, ex, want, f32 = net_data(kind)
    if final_relu:
        want, f32 = np.maximum(want, 0.0), np.maximum(f32, 0.0)
    net = F.VGGishHIP.from_module(model, final_relu=final_relu)
    got = net.forward(torch.from_numpy(ex).cuda())
    assert tuple(got.shape) == want.shape and got.dtype == torch.float32
    got = got.cpu().numpy()
    yard, err = O.rel_max(f32, want), O.rel_max(got, want)
    print(f"whole network, {kind}, final_relu {final_relu}: kernel {err:.3e}, float32 torch {yard:.3e}, gate {O.TOL_FACTOR * yard:.3e}")
    assert np.isfinite(got).all() and (not final_relu or got.min() >= 0.0)
    assert err <= O.TOL_FACTOR * yard
    if kind == "narrow":                             # an example alone: the same bits as in the batch
        alone = net.forward(torch.from_numpy(ex[1:2]).cuda()).cpu().numpy()
        assert np.array_equal(alone[0], got[1])


# ------------------------------------------------------------------ statistics and distance, end to end
@functools.lru_cache(maxsize=None)
def clip_sets():
    n = 3 * 48000
    a = np.stack([np.stack([O.mix(n, 100 + 2 * i, 48000), O.mix(n, 101 + 2 * i, 48000)]) for i in range(6)])
    k = np.ones(9) / 9.0                             # a low-pass (9-tap mean) and a gain
    b = np.stack([np.stack([0.6 * np.convolve(c, k, mode="same") for c in clip]) for clip in a]).astype(np.float32)
    return a, b


def test_score_end_to_end(F):
    from jen1_amd.audio import convert_audio
    a, b = clip_sets()
    model = O.VGGishModel(**O.NARROW, seed=33)
    fad = F.FrechetAudioDistance(F.VGGishHIP.from_module(model))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    sa, sb = fad.stats(ta, 48000), fad.stats(tb, 48000)
    assert sa.count == sb.count == 18
    got = fad.score(sa, sb)
    emb = {}
    for name, t in (("a", ta), ("b", tb)):
        x16 = convert_audio(t, 48000, 16000, 1, device="cuda").reshape(6, -1).cpu().numpy()
        for dt, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
            emb[name, dt] = O.run_model(model, np.concatenate([O.examples(r, dt) for r in x16]), tdt).astype(np.float64)
    want = O.frechet_np(emb["a", np.float64], emb["b", np.float64])
    f32 = O.frechet_np(emb["a", np.float32], emb["b", np.float32])
    yard, err = abs(f32 - want) / abs(want), abs(got - want) / abs(want)
    print(f"FAD end to end: kernel {got!r}, float64 {want!r}, relative {err:.3e}; float32 CPU chain {yard:.3e}, gate {O.TOL_FACTOR * yard:.3e}")
    assert got > 0
    assert err <= O.TOL_FACTOR * yard
    tr = float(np.trace(sa.cov()))
    d0 = fad.score(sa, sa)
    print(f"score(a, a) = {d0:.3e}, tr S = {tr:.3e}")
    assert abs(d0) <= 1e-9 * tr
    assert fad.score(ta, sb, 48000) == got          # a second run: the same bits
    assert torch.equal(fad.stats(ta, 48000).state, sa.state)


def test_stats_over_a_list_equals_the_merge_of_per_clip_stats(F):
    a, _ = clip_sets()
    fad = F.FrechetAudioDistance(F.VGGishHIP.from_module(O.VGGishModel(**O.NARROW, seed=33)))
    clips = [torch.from_numpy(a[0][:, :48000 * 3]).cuda(), torch.from_numpy(a[1][:, :50000]).cuda(), torch.from_numpy(a[2][:1, :100000]).cuda()]
    whole = fad.stats(clips, 48000)
    merged = F.FrechetStats(128)
    for c in clips:
        merged.merge(fad.stats(c, 48000))
    assert whole.count == 3 + 1 + 2
    assert torch.equal(whole.state.cpu(), merged.state.cpu())
    pairs = fad.stats(((c, 48000) for c in clips))
    assert torch.equal(pairs.state, whole.state)
    sd = whole.state_dict()
    assert fad.score(clips, F.FrechetStats.from_state_dict(sd), 48000) == fad.score(whole, whole)


def test_update_with_plain_embeddings_matches_numpy(F):
    rng = np.random.default_rng(4)
    e = rng.standard_normal((300, 128)).astype(np.float32)
    st = F.FrechetStats(128).update(torch.from_numpy(e).cuda()).update(torch.from_numpy(e[:0]).cuda())
    assert st.count == 300
    e64 = e.astype(np.float64)
    assert float(np.abs(st.mean() - e64.mean(0)).max()) <= 1e-12
    assert float(np.abs(st.cov() - np.cov(e64, rowvar=False)).max()) <= 1e-12


# ------------------------------------------------------------------ error paths
def test_error_paths(F, L):
    net = F.VGGishHIP.from_module(O.VGGishModel(**O.NARROW, seed=1))
    fad = F.FrechetAudioDistance(net)
    with pytest.raises(L.Jen1HipError):
        net.forward(torch.zeros(1, 96, 64))
    with pytest.raises(L.Jen1HipError):
        net.embed(torch.zeros(1, 1, 16000), 16000)
    with pytest.raises(ValueError):
        net.forward(torch.zeros(1, 96, 64, device="cuda", requires_grad=True))
    with pytest.raises(ValueError):
        fad.stats(torch.zeros(1, 1, 16000, device="cuda", requires_grad=True), 16000)
    with pytest.raises(TypeError):
        net.forward(torch.zeros(1, 96, 64, device="cuda", dtype=torch.float64))
    with pytest.raises(TypeError):
        F.vggish_examples(torch.zeros(1, 1, 16000, device="cuda", dtype=torch.float64), 16000)
    with pytest.raises(ValueError):
        net.forward(torch.zeros(1, 64, 96, device="cuda"))
    with pytest.raises(ValueError, match="no full example"):
        fad.stats(torch.zeros(2, 1, 15599, device="cuda"), 16000)
    with pytest.raises(ValueError):
        F.vggish_examples(torch.zeros(2, 1, 16000, device="cuda"), 16000, lengths=[16000])
