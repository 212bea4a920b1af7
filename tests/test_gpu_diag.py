"""GPU checks of the f64 whitening / centroid entries (include/sd_hip_diag.h) and of the device route of the "VBx-like" diarizer
(speech-diarization_amd/diag_gpu.py, diar_diag.py): known-answer inputs whose every product and sum is exact (equal to numpy bit for
bit), random inputs against numpy f64 under the summation bound, guard bands around every pointer, `whiten_l2_rows` against
`cluster.whiten_l2`, `resegment(device="cuda")` against the host route, the context spans against one-at-a-time embedding, and the
whole `diagnose` on a synthetic conversation.  Every kernel's launch label is asserted (tests/test_diag_rules.py holds the list)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import captured as CAP  # noqa: E402
import diag_cases as DC  # noqa: E402
import guarded as G  # noqa: E402
from launch_log import expect_launches  # noqa: E402

pytestmark = pytest.mark.gpu

STATS_LABELS = ["whiten_colsum_kernel", "whiten_mean_kernel", "whiten_gram_kernel", "whiten_gram_finish_kernel"]
R = 512                                                              # SD_WHITEN_ROWS: the statistics kernels' row block


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _ulp_ok(got, want64):
    """Each element within one f32 ulp of the f32-rounded f64 reference."""
    ref = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64)


# ------------------------------------------------------------------ statistics

def _integer_rows(n, d, seed, mean=None):
    """[A; -A] with |A| <= 2^10 (column sums zero), plus an integer mean row when given: every product and sum is an integer < 2^53."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-1024, 1025, size=(n // 2, d))
    x = np.concatenate([a, -a])[rng.permutation(n)]
    if mean is not None:
        x = x + mean
    return x.astype(np.int64)


@pytest.mark.parametrize("n,d", [(2, 4), (130, 20), (514, 192), (1030, 200), (R - 2, 36), (R, 36), (R + 2, 36), (2 * R + 2, 16)])
def test_stats_are_exact_on_integer_rows(dev, n, d):
    from speech_diarization_amd import ops
    xi = _integer_rows(n, d, n + d)
    x = torch.from_numpy(xi.astype(np.float32)).to(dev)
    with expect_launches(exactly=STATS_LABELS):                      # whiten_colsum_kernel whiten_mean_kernel whiten_gram_kernel whiten_gram_finish_kernel
        mean, gram = ops.whiten_stats(x)
    mean, gram = mean.cpu().numpy(), gram.cpu().numpy()
    assert mean.dtype == np.float64 and gram.shape == (d, d)
    assert np.array_equal(_bits(mean), _bits(np.zeros(d)))
    assert np.array_equal(_bits(gram), _bits((xi.T @ xi).astype(np.float64)))
    assert np.array_equal(_bits(gram), _bits(gram.T.copy()))
    m2, g2 = ops.whiten_stats(x)
    assert np.array_equal(_bits(m2.cpu().numpy()), _bits(mean)) and np.array_equal(_bits(g2.cpu().numpy()), _bits(gram))


@pytest.mark.parametrize("n,d", [(64, 20), (1024, 192)])
def test_stats_are_exact_with_an_integer_mean(dev, n, d):
    """n a power of two and column sums n . mean: the mean is an exact integer and so is every centred value."""
    from speech_diarization_amd import ops
    m = np.random.default_rng(d).integers(-500, 501, size=d)
    xi = _integer_rows(n, d, n, mean=m)
    mean, gram = ops.whiten_stats(torch.from_numpy(xi.astype(np.float32)).to(dev))
    xc = xi - m
    assert np.array_equal(mean.cpu().numpy(), m.astype(np.float64))
    assert np.array_equal(_bits(gram.cpu().numpy()), _bits((xc.T @ xc).astype(np.float64)))


@pytest.mark.parametrize("scale", [1e-3, 1.0, 300.0])
@pytest.mark.parametrize("n", [40, 300, 2000])
def test_stats_on_random_rows_stay_under_the_summation_bound(dev, n, scale):
    """|gram - ref| <= 4 n 2^-53 (|Xc|^T |Xc|) elementwise: the products are exact to one f64 rounding each, so what is left is the
    order of n additions, on each side (numpy's blocked dot is a reordered sum as well)."""
    from speech_diarization_amd import ops
    rng = np.random.default_rng(n)
    x = ((rng.standard_normal((n, 192)) * rng.uniform(0.1, 3.0, 192) + rng.standard_normal(192)) * scale).astype(np.float32)
    mean, gram = ops.whiten_stats(torch.from_numpy(x).to(dev))
    x64 = x.astype(np.float64)
    mref = x64.mean(0)
    xc = x64 - mref
    ref = xc.T @ xc
    bound = 4 * n * 2.0 ** -53 * (np.abs(xc).T @ np.abs(xc))
    err = np.abs(gram.cpu().numpy() - ref)
    print(f"n={n} scale={scale}: max err / bound = {(err / bound).max():.3f}, max |mean - ref| = {np.abs(mean.cpu().numpy() - mref).max():.2e}")
    assert np.all(err <= bound)
    assert np.all(np.abs(mean.cpu().numpy() - mref) <= 2 * n * 2.0 ** -53 * np.abs(x64).mean(0))       # n additions on each side


# ------------------------------------------------------------------ the transform

def _exact_apply_case(n, d, seed):
    """W = a signed permutation times powers of two; x - mean has four non-zero entries, sized so that every one of them comes out of
    W as +-2^m: the norm is 2^(m + 1) and nothing is rounded anywhere."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(d)
    e = rng.integers(0, 4, size=d)
    w = np.zeros((d, d))
    w[np.arange(d), perm] = rng.choice([-1.0, 1.0], d) * 2.0 ** e
    mean = rng.integers(-8, 9, size=d).astype(np.float64)
    x = np.tile(mean, (n, 1))
    for i in range(n):
        cols = rng.choice(d, 4, replace=False)
        x[i, cols] += rng.choice([-1.0, 1.0], 4) * 2.0 ** (int(rng.integers(3, 9)) - e[cols])
    return x.astype(np.float32), mean, w


@pytest.mark.parametrize("n,d", [(17, 4), (130, 20), (514, 192), (33, 200)])
def test_apply_is_exact_on_signed_permutations(dev, n, d):
    from speech_diarization_amd import ops
    x, mean, w = _exact_apply_case(n, d, n + d)
    assert np.array_equal(x.astype(np.float64), x.astype(np.float64).astype(np.float32).astype(np.float64))
    with expect_launches(exactly=["whiten_apply_kernel"]):
        got = ops.whiten_apply(torch.from_numpy(x).to(dev), torch.from_numpy(mean).to(dev), torch.from_numpy(w).to(dev), eps_add=0.0)
    v = (x.astype(np.float64) - mean) @ w
    nrm = np.sqrt((v * v).sum(1, keepdims=True))
    assert np.all(np.log2(nrm) == np.round(np.log2(nrm)))            # powers of two
    want = (v / nrm).astype(np.float32)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(_bits(got.cpu().numpy())[want != 0], _bits(want)[want != 0])


@pytest.mark.parametrize("n,d", [(130, 20), (300, 192), (1000, 256)])
def test_apply_on_random_rows_is_within_one_ulp(dev, n, d):
    """eps_add = 1e-9, a random f64 W without symmetry: the f64 error of a d-term sum is far below half an f32 ulp, so at most the
    one rounding flips."""
    from speech_diarization_amd import ops
    rng = np.random.default_rng(n + d)
    x = (rng.standard_normal((n, d)) * 30.0 + 5.0).astype(np.float32)
    mean = x.astype(np.float64).mean(0)
    w = rng.standard_normal((d, d)) / np.sqrt(d)
    got = ops.whiten_apply(torch.from_numpy(x).to(dev), torch.from_numpy(mean).to(dev), torch.from_numpy(w).to(dev), eps_add=1e-9).cpu().numpy()
    v = (x.astype(np.float64) - mean) @ w
    want = v / (np.linalg.norm(v, axis=1, keepdims=True) + 1e-9)
    ok = _ulp_ok(got, want)
    print(f"n={n} d={d}: {int((got != want.astype(np.float32)).sum())} of {got.size} elements one ulp off")
    assert ok.all(), np.abs(got - want).max()


# ------------------------------------------------------------------ centres

def _exact_centroid_case(d, seed):
    """Labels 0 .. 4 with 2, 8, 16, 0 and 64 rows (label 3 is empty), 30 noise rows (-1) and 5 rows of an out-of-range label: the rows
    of a label are its mean (four entries +-2^p) plus [B; -B], shuffled among the others."""
    rng = np.random.default_rng(seed)
    rows, labels, means = [], [], {}
    for c, cnt in enumerate([2, 8, 16, 0, 64]):
        m = np.zeros(d)
        if cnt:
            m[rng.choice(d, 4, replace=False)] = rng.choice([-1.0, 1.0], 4) * 2.0 ** int(rng.integers(0, 6))
            b = rng.integers(-512, 513, size=(cnt // 2, d)).astype(np.float64)
            rows.append(np.concatenate([b, -b]) + m)
            labels += [c] * cnt
        means[c] = m
    rows.append(rng.integers(-512, 513, size=(35, d)).astype(np.float64))
    labels += [-1] * 30 + [7] * 5
    x, labels = np.concatenate(rows), np.asarray(labels, np.int32)
    p = rng.permutation(len(labels))
    return x[p].astype(np.float32), labels[p], means


@pytest.mark.parametrize("d", [4, 20, 192, 256])
def test_centroids_are_exact_on_integer_rows(dev, d):
    from speech_diarization_amd import ops
    x, labels, means = _exact_centroid_case(d, d)
    with expect_launches(exactly=["label_centroids_kernel"]):
        cen, count = ops.label_centroids(torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev), 5, eps_add=0.0)
    cen, count = cen.cpu().numpy(), count.cpu().numpy()
    assert count.tolist() == [2, 8, 16, 0, 64] and count.dtype == np.int32
    for c in range(5):
        m = means[c]
        want = (m / np.sqrt((m * m).sum())).astype(np.float32) if count[c] else np.zeros(d, np.float32)
        assert np.array_equal(cen[c], want), c
    one, cnt1 = ops.label_centroids(torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev), 1, eps_add=0.0)       # k = 1
    assert np.array_equal(one.cpu().numpy(), cen[:1]) and cnt1.tolist() == [2]


@pytest.mark.parametrize("n,d,k", [(130, 20, 3), (1000, 192, 8), (3000, 256, 40)])
def test_centroids_on_random_rows_are_within_one_ulp(dev, n, d, k):
    from speech_diarization_amd import ops
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((n, d)) * 30.0 + 5.0).astype(np.float32)
    labels = rng.integers(-1, k, size=n).astype(np.int32)
    cen, count = ops.label_centroids(torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev), k)
    want = np.zeros((k, d))
    for c in range(k):
        m = x[labels == c].astype(np.float64).mean(0)
        want[c] = m / (np.linalg.norm(m) + 1e-9)
    assert count.cpu().tolist() == [int((labels == c).sum()) for c in range(k)]
    assert _ulp_ok(cen.cpu().numpy(), want).all()


# ------------------------------------------------------------------ guard bands

@pytest.mark.parametrize("n,d,ld", [(130, 20, 24), (514, 190, 192)])
def test_no_entry_leaves_its_buffers(dev, n, d, ld):
    """Every pointer of the three entries inside guard bands; the padding columns of x hold 0xFF bytes (NaN), the output padding
    columns a poison that must survive; the workspace is exactly sd_whiten_stats_workspace_bytes."""
    from speech_diarization_amd import _native as N
    lib = N.load()
    rng = np.random.default_rng(n)
    xv = (rng.standard_normal((n, d)) * 30.0).astype(np.float32)
    xp = np.full((n, ld), np.nan, np.float32)
    xp.view(np.uint8)[:] = 0xFF
    xp[:, :d] = xv
    ldg, ldw, ldo, k = d + 3, d + 1, ld, 5
    labels = rng.integers(-1, k + 1, size=n).astype(np.int32)
    x = G.guarded_from(torch.from_numpy(xp), dev, "x")
    mean = G.guarded(d * 8, 0x7B, dev, "mean")
    gram = G.guarded(d * ldg * 8, 0x7B, dev, "gram")
    need = int(lib.sd_whiten_stats_workspace_bytes(n, d))
    ws = G.guarded(need, 0xFF, dev, "ws")
    N.check(CAP.call("sd_whiten_stats_f64", x.ptr, ld, n, d, mean.ptr, gram.ptr, ldg, ws.ptr, need), "sd_whiten_stats_f64")
    torch.cuda.synchronize()
    g = gram.view(torch.float64, d, ldg)
    G.assert_columns_keep(g, 0, d, 0x7B, "gram")
    m_got, g_got = mean.view(torch.float64).cpu().numpy(), g[:, :d].cpu().numpy()
    xc = xv.astype(np.float64) - xv.astype(np.float64).mean(0)
    assert np.isfinite(m_got).all() and np.isfinite(g_got).all()
    assert np.abs(g_got - xc.T @ xc).max() <= 4 * n * 2.0 ** -53 * (np.abs(xc).T @ np.abs(xc)).max()

    w_np = rng.standard_normal((d, ldw))
    w = G.guarded_from(torch.from_numpy(w_np), dev, "w")
    out = G.guarded(n * ldo * 4, 0x7B, dev, "out")
    N.check(CAP.call("sd_whiten_apply_f64", x.ptr, ld, n, d, mean.ptr, w.ptr, ldw, 1e-9, out.ptr, ldo), "sd_whiten_apply_f64")
    torch.cuda.synchronize()
    o = out.view(torch.float32, n, ldo)
    G.assert_columns_keep(o, 0, d, 0x7B, "out")
    v = (xv.astype(np.float64) - m_got) @ w_np[:, :d]
    assert _ulp_ok(o[:, :d].cpu().numpy(), v / (np.linalg.norm(v, axis=1, keepdims=True) + 1e-9)).all()

    lab = G.guarded_from(torch.from_numpy(labels), dev, "labels")
    cen = G.guarded(k * ldo * 4, 0x7B, dev, "centres")
    cnt = G.guarded(k * 4, 0x7B, dev, "count")
    N.check(CAP.call("sd_label_centroids_f32", x.ptr, ld, n, d, lab.ptr, k, 1e-9, cen.ptr, ldo, cnt.ptr), "sd_label_centroids_f32")
    torch.cuda.synchronize()
    c = cen.view(torch.float32, k, ldo)
    G.assert_columns_keep(c, 0, d, 0x7B, "centres")
    assert torch.isfinite(c[:, :d]).all() and cnt.view(torch.int32).cpu().tolist() == [int((labels == j).sum()) for j in range(k)]
    G.assert_guards_intact(x, mean, gram, ws, w, out, lab, cen, cnt)


# ------------------------------------------------------------------ the driver

@pytest.mark.parametrize("n", [40, 300, 2000])
@pytest.mark.parametrize("kind", ["planted", "isotropic"])
def test_whiten_l2_rows_equals_the_host_function(dev, n, kind):
    """Rows within 2^-22: one f32 rounding of an entry <= 1 is 2^-25 and the reordered f64 sums stay near 1e-9; w w^T within the
    project's 1e-6 for this function (tests/test_glue_golden.py)."""
    from speech_diarization_amd import cluster, diag_gpu
    if kind == "planted":
        X, _ = DC.planted_lowrank(n, 4, 8, 0.3, n)
    else:
        X = (np.random.default_rng(n).standard_normal((n, DC.D)) * 30.0).astype(np.float32)
    with expect_launches(exactly=STATS_LABELS + ["whiten_apply_kernel"]):
        got = diag_gpu.whiten_l2_rows(torch.from_numpy(X).to(dev))
    assert got.device.type == "cuda" and got.dtype == torch.float32
    got = got.cpu().numpy().astype(np.float64)
    want = cluster.whiten_l2(X)
    print(f"n={n} {kind}: rows {np.abs(got - want).max():.2e}, w w^T {np.abs(got @ got.T - want @ want.T).max():.2e}")
    assert np.abs(got - want).max() <= 2.0 ** -22
    assert np.abs(got @ got.T - want @ want.T).max() <= 1e-6


# ------------------------------------------------------------------ resegment on the device against the host route

def _renamed(host, device_labels):
    """The bijection host cluster label -> device cluster label (None when the partitions differ; noise must map to noise).
    scikit-learn's labels follow its merge tree, the device AHC numbers clusters by first appearance and the device HDBSCAN hands
    scikit-learn a tree with its edges in another order, so the NAMES of equal partitions differ."""
    pairs = set(zip(host.tolist(), device_labels.tolist()))
    if len({a for a, _ in pairs}) != len(pairs) or len({b for _, b in pairs}) != len(pairs):
        return None
    if any((a == -1) != (b == -1) for a, b in pairs):
        return None
    return dict(pairs)


# One of the 16 combinations is replaced by the same shape under another seed.  (130, 4, 8, 0.3, 2) with "hdbscan" and whitening: row 20
# hangs on the spanning tree by TWO edges of exactly the same float64 weight (its own core distance 0.29997925..., to rows 12 and 56), so
# the float64 margin of the comparison that decides it is 0: whichever edge scikit-learn's argsort meets first makes the row noise or a
# member of cluster 1.  The host route and the device route hand over the edges in different orders; the difference shows on the CPU
# as well, with numpy operators in place of the kernels and with float64 rows (the tie caveat in the docstring of hdbscan_gpu.py).
REPLACED = {((130, 4, 8, 0.3, 2), "hdbscan", 1): (130, 4, 8, 0.3, 12)}


@pytest.mark.parametrize("whiten", [0, 1])
@pytest.mark.parametrize("method", ["agglo", "hdbscan"])
@pytest.mark.parametrize("case", DC.RESEGMENT_CASES, ids=lambda c: f"n{c[0]}")
def test_resegment_on_the_device_equals_the_host_route(dev, case, method, whiten):
    """Same partition, same path and same merged segments; scores within 1e-4 of the largest score.  The cluster NUMBERS of the two
    routes are compared through their bijection (see `_renamed`): under "hdbscan" too the numbers follow the order of the tree's
    edges, which the two routes build differently (measured: (48, 3, 6, 0.3, 1) without whitening comes out as 1 2 0 and 2 1 0)."""
    from speech_diarization_amd import diar_diag as dd
    case = REPLACED.get((case, method, whiten), case)
    X, _ = DC.planted_lowrank(*case)
    n = len(X)
    segs = [[i * 1.0, i * 1.0 + 0.8] for i in range(n)]
    host = dd.resegment(X, segs, cluster=method, whiten=whiten)
    got = dd.resegment(torch.from_numpy(X).to(dev), segs, cluster=method, whiten=whiten, device=dev)
    name = _renamed(host["labels"], got["labels"])
    assert name is not None, f"{int((host['labels'] != got['labels']).sum())} of {n} labels differ and the partitions are not the same"
    # centre i of a route belongs to the i-th smallest non-noise label
    h_uniq = sorted(u for u in set(host["labels"].tolist()) if u != -1)
    g_uniq = sorted(u for u in set(got["labels"].tolist()) if u != -1)
    col = np.asarray([g_uniq.index(name[u]) for u in h_uniq])        # host centre index -> device centre index
    assert np.array_equal(col[host["final_labels"]], got["final_labels"])
    hs, gs = np.asarray(host["scores"], np.float64), got["scores"].cpu().numpy().astype(np.float64)[:, col]
    diff, top = np.abs(hs - gs).max(), np.abs(hs).max()
    print(f"{case} {method} whiten={whiten}: K={len(h_uniq)}, max score difference {diff:.2e} of {top:.2f}")
    assert diff <= 1e-4 * top
    assert np.abs(got["centers"][col] - host["centers"]).max() <= 1e-5      # unit means of rows that agree to 2^-22, over a norm >= 0.1
    spk = {f"SPK_{i}": f"SPK_{j}" for i, j in enumerate(col.tolist())}
    assert [dict(s, speaker=spk[s["speaker"]]) for s in host["segments"]] == got["segments"]
    tol = 192 * 2.0 ** -24 + 2.0 ** -20                              # an f32 dot product of 192 terms at its worst, over rows that agree to 2^-22
    assert np.abs(got["adjacent"] - host["adjacent"]).max() <= tol and np.abs(got["nonadjacent"] - host["nonadjacent"]).max() <= tol


# ------------------------------------------------------------------ spans and the whole pipeline

_CACHE = {}


def _encoder(dev):
    from speech_diarization_amd import synth
    from speech_diarization_amd.speech_encode import HipEcapaEncoder
    if "enc" not in _CACHE:
        _CACHE["enc"] = HipEcapaEncoder(synth.make_ecapa_state_dict(1234), dev)
    return _CACHE["enc"]


def test_context_spans_embed_as_each_piece_alone(dev):
    """A 30 s conversation with hand-placed segments: one that needs tiling (0.1 s + 2 x 0.1 s context < 0.4 s), one clamped at each
    end.  Against `encode_batch` of each piece alone (B = 1): cosine distance < 1e-6, the packed route's own bar."""
    from speech_diarization_amd import diar_diag as dd
    from speech_diarization_amd import synth
    enc = _encoder(dev)
    y = synth.synthetic_conversation(30.0, 2, seed=3).wav
    segs = [[0.05, 1.3], [4.0, 4.1], [7.25, 9.8], [12.0, 12.6], [28.9, 29.95]]
    ctx = 0.1
    got = dd.embed_segments_with_context(y, 16000, segs, pad_ctx=ctx, encoder=enc)
    starts, lengths, tile_to = dd.context_spans(segs, len(y), 16000, ctx)
    assert starts[0] == 0 and starts[-1] + lengths[-1] == len(y) and tile_to.tolist() == [0, 6400, 0, 0, 0] and 4799 <= lengths[1] <= 4800
    alone = []
    for s, n, t in zip(starts.tolist(), lengths.tolist(), tile_to.tolist()):
        a = y[s:s + n]
        if t:
            a = np.tile(a, -(-t // n))[:t]
        alone.append(enc.encode_batch(torch.from_numpy(a.copy())[None]).squeeze(1).cpu().numpy())
    alone = np.concatenate(alone)
    cd = 1.0 - (got * alone).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(alone, axis=1))
    print(f"spans vs alone: max cosine distance {cd.max():.2e}")
    assert got.shape == (5, 192) and np.isfinite(got).all() and cd.max() < 1e-6
    dev_rows = dd.embed_segments_with_context(y, 16000, segs, pad_ctx=ctx, encoder=enc, to_host=False)
    assert dev_rows.device.type == "cuda" and np.array_equal(dev_rows.cpu().numpy(), got)


def test_diagnose_end_to_end_on_a_conversation(dev, tmp_path):
    """120 s, three synthetic voices: the device route writes the three files and equals the host route fed by the same GPU
    encoder, on agglo without whitening (a random-init network gives no speaker structure that survives whitening; planted rows
    cover that part above)."""
    from speech_diarization_amd import diar_diag as dd
    from speech_diarization_amd import synth
    enc = _encoder(dev)
    conv = synth.synthetic_conversation(120.0, 3, seed=5, turn_s=(1.0, 2.0))
    probs = dd.silero_probs_raw(conv.wav, 16000)
    kw = dict(cluster="agglo", whiten=0, encoder=enc)
    host = dd.diagnose(conv.wav, 16000, probs, device=None, out_dir=str(tmp_path / "host"), **kw)
    got = dd.diagnose(conv.wav, 16000, probs, device=dev, out_dir=str(tmp_path / "dev"), **kw)
    assert len(got["vad_segments"]) >= 30 and got["vad_segments"] == host["vad_segments"]
    name = _renamed(host["labels"], got["labels"])
    assert name is not None
    h_uniq = sorted(set(host["labels"].tolist()))
    g_uniq = sorted(set(got["labels"].tolist()))
    spk = {f"SPK_{i}": f"SPK_{g_uniq.index(name[u])}" for i, u in enumerate(h_uniq)}
    assert [dict(s, speaker=spk[s["speaker"]]) for s in host["segments"]] == got["segments"]
    for kind in ("json", "srt", "csv"):
        assert os.path.getsize(got["paths"][kind]) > 0
    if all(k == v for k, v in spk.items()):                          # the same names: the files are the same bytes
        for kind in ("json", "srt", "csv"):
            assert open(got["paths"][kind], "rb").read() == open(host["paths"][kind], "rb").read()
    print(f"{len(got['vad_segments'])} VAD segments, {len(g_uniq)} clusters, {len(got['segments'])} merged segments, speakers {got['speakers']}")
