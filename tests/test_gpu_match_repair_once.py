"""The matcher's certified, merged repair of the second best (k_match.hip: mf_repair_accept, the `group` lambda of
match_v2_body; docs/match_repair_once.md) against the CPU oracle byte for byte (result record and pass-1 correspondence
list), through the split form (k_match_split: four resident "to" tiles, two decode passes per group) and the fused kernel
(two tiles, one pass).

A column that passes NNDR against the scan's optimistic second best is decided again on its best row's class: certified on
the Hamming distance p over the first four dwords of the class's other rows where that suffices, exactly otherwise.  The
cases plant, for chosen columns, a best row at distance 20 and a class mate the certificate cannot decide on:
  * "half": the mate is 4 bits away in dwords 0..3 and 96 in dwords 4..7 (p = 4, d = 100): uncertified at nndr 0.6
    (20 > 0.6 * 4), and the exact decision stays ACCEPT (20 <= 0.6 * 100) -- a failed certificate must not reject;
  * "all": the mate is 12 bits away in each half (p = 12, d = 24): uncertified, and the exact decision is REJECT
    (20 > 0.6 * 24) where the optimistic one accepted.
Everything else is random against random (distances about 100 and up at these sizes: rejected at 0.6).  The K = 500 cases
fill a wavefront's group (columns 32 w ... and 32 (w + 4) ... in pass 0, 32 (w + 8) ... and 32 (w + 12) ... in pass 1) with
a chosen number of repairing columns: at most 64 move into one set of lanes, 65 and more repair pass by pass.
The file pins behaviour and defines none: every case passes on the build before this change."""
import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, synth

from test_gpu_match_edges import _check, _params
from test_gpu_match_second_best import _flipped, _frame

pytestmark = pytest.mark.gpu

D1 = 20


def _flipped_in(rng, row, lo, hi, n):
    """`row` (uint8 bytes) with n distinct bits of bytes lo..hi-1 inverted."""
    out = row.copy()
    for bit in rng.choice(np.arange(lo * 8, hi * 8), size=n, replace=False):
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


def _mate(rng, col, kind):
    if kind == "half":
        return _flipped_in(rng, _flipped_in(rng, col, 0, 16, 4), 16, 32, 96)
    assert kind == "all"
    return _flipped_in(rng, _flipped_in(rng, col, 0, 16, 12), 16, 32, 12)


def _row(tile, h, reg):
    """The "from" row that register `reg` of lane half h holds in tile `tile` (the class map of top2_update16)."""
    return 32 * tile + (reg & 3) + 8 * (reg >> 2) + 4 * h


def _pair(seed, kf, kt, plants):
    """A random pair in which, for every (t, best, mate, kind) of `plants`, "from" row `best` is D1 bits from column t and
    row `mate` (None: no mate) is the class mate of `kind`.  Returns (from, to, accepted pass-1 correspondences)."""
    rng = np.random.default_rng(seed)
    a, b = _frame(rng, kf, 32), _frame(rng, kt, 32)
    da, used, cols, n_acc = a.desc.copy(), set(), set(), 0
    for t, best, mate, kind in plants:
        assert t < kt and t not in cols and best < kf and best not in used and (mate is None or (mate < kf and mate not in used))
        cols.add(t); used.add(best)
        da[best] = _flipped(rng, b.desc[t], D1)
        if mate is not None:
            used.add(mate)
            da[mate] = _mate(rng, b.desc[t], kind)
        n_acc += mate is None or kind == "half"
    return _abi.FeatureArrays(da, a.xyz, a.kpts), b, n_acc


def _position_plants(k, kind):
    """The best row in every position the class map distinguishes: both lane halves; registers 0, 14 (the mate in the
    same class, registers 13 and 1) and 15 (a class of its own: the mate, register 12, is in the scan's second best
    already); the first tile and the last full one; at K = 130 the ragged tile (rows 128, 129: the class's other rows are
    >= Kf)."""
    plants, t = [], 1
    step = (k - 2) // 14
    for tile in (0, k // 32 - 1):
        for h in (0, 1):
            for rb, rm in ((0, 13), (14, 1), (15, 12)):
                plants.append((t, _row(tile, h, rb), _row(tile, h, rm), kind))
                t += step
    if k & 31:
        best = k - 2 if kind == "half" else k - 1              # (the two kinds the two ways round)
        plants.append((t, best, 2 * k - 3 - best, kind))
    return plants


def _group_columns(w, n0, n1, rng):
    """n0 columns of wavefront w's pass 0 and n1 of its pass 1 at K = 500 (16 column tiles, wavefront w owns tiles w, w + 4,
    w + 8, w + 12; a pass decides two of them, one per lane half), spread over both lane halves."""
    p0 = np.concatenate([np.arange(32) + 32 * w, np.arange(32) + 32 * (w + 4)])
    p1 = np.concatenate([np.arange(32) + 32 * (w + 8), np.arange(32) + 32 * (w + 12)])
    p1 = p1[p1 < 500]
    return sorted(rng.choice(p0, size=n0, replace=False).tolist()), sorted(rng.choice(p1, size=n1, replace=False).tolist())


def _filled_group(seed, n0, n1, w=0):
    """K = 500: wavefront w's group with exactly n0 + n1 repairing columns (n0 in pass 0), some of them with mates the
    certificate cannot decide on, in both passes: the columns of pass 1 repair in other lanes when n0 + n1 <= 64."""
    rng = np.random.default_rng(seed)
    c0, c1 = _group_columns(w, n0, n1, rng)
    rows = rng.permutation(500 // 32 * 2)                      # a (tile, half) of its own per column: distinct classes
    plants = []
    for n, t in enumerate(c0 + c1):
        tile, h = int(rows[n % len(rows)]) >> 1, int(rows[n % len(rows)]) & 1
        reg = 3 * (n // len(rows))                             # registers 0, 3, 6, 9 with mates 1, 4, 7, 10
        kind = ("half", "all", None, None, None)[n % 5]
        plants.append((t, _row(tile, h, reg), _row(tile, h, reg + 1) if kind else None, kind))
    return _pair(seed + 1, 500, 500, plants)


def _all_accepting(seed):
    """K = 500, frame B = frame A's rows with 3 bits flipped each: every column repairs (128 per group)."""
    rng = np.random.default_rng(seed)
    a = _frame(rng, 500, 32)
    b = _frame(rng, 500, 32)
    db = np.stack([_flipped(rng, a.desc[(7 * i + 3) % 500], 3) for i in range(500)])
    return a, _abi.FeatureArrays(db, b.xyz, b.kpts), 500


def _forty_percent(seed):
    A, B, _, _ = synth.make_pairs(seed, 1, k=500, cols=32, true_frac=1.0)
    return A[0], B[0], None


def _cases_06():
    c = []
    for k in (64, 96, 130):
        c.append(("half_k%d" % k, *_pair(6100 + k, k, k, _position_plants(k, "half"))))
        c.append(("all_k%d" % k, *_pair(6200 + k, k, k, _position_plants(k, "all"))))
    c.append(("half_k500", *_pair(6300, 500, 500, _position_plants(500, "half"))))
    c.append(("all_k500", *_pair(6301, 500, 500, _position_plants(500, "all"))))
    # degenerate "from" frames: Kf = 1 (no second best: nothing is accepted), Kf = 2 (both rows in one class: no second
    # best outside it, the scan's is absent)
    c.append(("kf_1", *_pair(6310, 1, 40, [(0, 0, None, None)])[:2], 0))
    c.append(("kf_2_half", *_pair(6311, 2, 40, [(3, 0, 1, "half")])))
    c.append(("kf_2_all", *_pair(6312, 2, 40, [(35, 1, 0, "all")])))
    return c


def _cases_merge():
    c = [("overflow_128", *_all_accepting(6400)), ("forty_percent", *_forty_percent(6401))]
    c.append(("exactly_64", *_filled_group(6410, 40, 24)))
    c.append(("exactly_65", *_filled_group(6420, 40, 25)))
    c.append(("exactly_64_w3", *_filled_group(6430, 50, 14, w=3)))     # (wavefront 3: its last tile has 20 columns)
    c.append(("one_and_63", *_filled_group(6440, 1, 63, w=1)))
    c.append(("pass_1_only", *_filled_group(6450, 0, 30, w=2)))
    return c


def _twins(seed, k, kt):
    """Every "from" row r with (r & 8) == 0 copied to row r + 8 (the same lane half: the same class, but for rows 19 / 23
    whose twins 27 / 31 are classes of their own)."""
    rng = np.random.default_rng(seed)
    a, b = _frame(rng, k, 32), _frame(rng, kt, 32)
    d = a.desc.copy()
    for r in range(k - 8):
        if not r & 8:
            d[r + 8] = d[r]
    return _abi.FeatureArrays(d, a.xyz, a.kpts), b


def _cases_ties():
    return [("twins_%d" % k, *_twins(6500 + k, k, k), None) for k in (64, 96, 130)]


def _cases_negative():
    """nndr < 0 accepts d1 = d2 = 0 only: columns that ARE a twinned "from" row (the lower twin is taken); a column equal to
    an untwinned row (K = 130: rows 128, 129) has d2 > 0 and is rejected."""
    c = []
    for k in (64, 96, 130):
        a, b = _twins(6600 + k, k, k)
        db = b.desc.copy()
        src = [0, 5, 16, 19, 23, k - 32 + 1, k - 32 + 22]
        for n, r in enumerate(src):
            db[3 + 9 * n] = a.desc[r]
        n_acc = len(src)
        if k == 130:
            db[2], db[127] = a.desc[128], a.desc[129]
        c.append(("negative_%d" % k, a, _abi.FeatureArrays(db, b.xyz, b.kpts), n_acc))
    return c


def _get(builder, cache={}):
    if builder not in cache:
        cache[builder] = builder()
    return cache[builder]


def _run(monkeypatch, oracle, split, nndr, cases):
    A, B = [c[1] for c in cases], [c[2] for c in cases]
    expect = {i: c[3] for i, c in enumerate(cases) if c[3] is not None}
    _check(monkeypatch, oracle, split, _params(nndr), A, B, expect)


@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_uncertified_accept_alone(monkeypatch, oracle, split):
    # one case alone, so that it fails on its own when a failed certificate rejects
    _run(monkeypatch, oracle, split, 0.6, _get(_cases_06)[:1])


@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_uncertified_columns_in_every_position(monkeypatch, oracle, split):
    _run(monkeypatch, oracle, split, 0.6, _get(_cases_06)[1:])


@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_merge_fits_and_overflows(monkeypatch, oracle, split):
    _run(monkeypatch, oracle, split, 0.6, _get(_cases_merge))


@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_ties_at_nndr_one(monkeypatch, oracle, split):
    _run(monkeypatch, oracle, split, 1.0, _get(_cases_ties) + _get(_cases_merge)[:2])


@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_negative_nndr_takes_the_exact_path(monkeypatch, oracle, split):
    _run(monkeypatch, oracle, split, -0.5, _get(_cases_negative) + [c[:3] + (0,) for c in _get(_cases_06)[:2]])


@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_shuffled_batch_with_unrelated_pairs(monkeypatch, oracle, split):
    rng = np.random.default_rng(6700)
    cases = list(_get(_cases_06)) + list(_get(_cases_merge))
    for i in range(12):
        cases.append(("unrelated_%d" % i, _frame(rng, 500, 32), _frame(rng, 500, 32), 0))
    cases = [cases[i] for i in rng.permutation(len(cases))]
    _run(monkeypatch, oracle, split, 0.6, cases)


def test_through_the_step_pair(monkeypatch, oracle):
    """The K = 500 cases as two robots' keyframe stores through sf_step_issue / sf_step_retire in the split form: every
    match's verdict and every accepted record are the oracle's."""
    import torch
    from multi_robot_slam_separators_amd import lib
    monkeypatch.setenv("SF_FUSED", "2")
    cases = [c for c in list(_get(_cases_merge)) + list(_get(_cases_06)) if len(c[1].desc) == 500 and len(c[2].desc) == 500]
    A, B, _, _ = synth.make_pairs(6800, 3, k=500, cols=32, true_frac=1.0)
    pairs = [(c[1], c[2]) for c in cases] + list(zip(A, B))
    n_kf, dim = len(pairs), 128
    rng = np.random.default_rng(6801)
    nv_a = rng.normal(size=(n_kf, dim)); nv_a /= np.linalg.norm(nv_a, axis=1, keepdims=True)
    nv_b = nv_a + 0.002 * rng.normal(size=(n_kf, dim)); nv_b /= np.linalg.norm(nv_b, axis=1, keepdims=True)
    p = _params(0.6)
    p.netvlad_dimensions = dim
    p.netvlad_max_matches_nb = n_kf
    p.max_features = 500
    dev = torch.device("cuda:0")

    def up(x):
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.view(np.uint8) if x.dtype.fields else x).to(dev)

    with lib.SeparatorFinder(p) as f:
        f.set_stream(torch.cuda.current_stream().cuda_stream)
        T = [up(np.stack([getattr(pr[s], key) for pr in pairs])) for s in (0, 1) for key in ("desc", "xyz", "kpts")]
        sa = f.store_add_keyframes_device(n_kf, 500, 32, T[0].data_ptr(), T[1].data_ptr(), T[2].data_ptr())
        sb = f.store_add_keyframes_device(n_kf, 500, 32, T[3].data_ptr(), T[4].data_ptr(), T[5].data_ptr())
        torch.cuda.synchronize()
        f.nn_append_received(nv_a)
        f.nn_append_local(nv_b)
        f.step_issue(sa, sb)
        matches, rom, recs, info = f.step_retire(copy=True)
        assert info["n_matches"] == n_kf
        n_ok = 0
        for i in range(n_kf):
            il, io = int(matches["idx_local"][i]), int(matches["idx_other"][i])
            o = oracle.estimate_transform(p, pairs[io][0], pairs[il][1])
            assert (rom[i] >= 0) == bool(o["success"]), i
            if o["success"]:
                n_ok += 1
                assert recs[rom[i]].tobytes() == o.tobytes(), i
        assert n_ok >= 3
