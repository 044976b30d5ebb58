"""The pruning bound of the batched rotation search (csrc/rotsearch.hip, rotation_search_batch_kernel), probed angle by
angle through the caller's own angle tables.

The kernel does not export its bounds.  A probe (tests/rotsearch_ref.py, tests/rotsearch_cases.py; that the probes are fair
is tests/test_rotation_bound_cpu.py's matter) launches the search with the 16 coarse angles [A] x 15 + [B], and with
[B] + [A] x 15, where the long-double score of A is that of B times 1 + eps.  With a sound bound B is scored and wins; if
the bound of B exceeded s(A), B would never be scored and the record would name an A.  Sixteen entries: every wave's
second item matters.  Every coarse angle's fine grid is the angle itself, so the record's status is OK and the fine score
has to repeat the coarse one bit for bit.

What a probe cannot see: an overshoot of the bound smaller than eps plus the gap the bound leaves by design at that
geometry (the census of DESIGN.md section 5).  Expected values come from the long-double reference alone."""
import numpy as np
import pytest

import rotsearch_cases as rc
import rotsearch_ref as ref

pytestmark = pytest.mark.gpu

K, CSCORE, NF, J, FSCORE, STATUS, EVALS, FEVALS = 6, 7, 8, 9, 10, 11, 12, 13


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from icpmi import _lib
    assert (K, CSCORE, NF, J, FSCORE) == (_lib.RSREC_K, _lib.RSREC_CSCORE, _lib.RSREC_NF, _lib.RSREC_J, _lib.RSREC_FSCORE)
    assert (STATUS, EVALS, FEVALS) == (_lib.RSBREC_STATUS, _lib.RSBREC_EVALS, _lib.RSBREC_FEVALS)


class Tables:
    """What RotationSearchBatch reads of its ``tables``: the angles on the host, their cos / sin on the device.  ``fine``:
    one grid per coarse angle ([K, L]); None: the coarse angle itself."""

    def __init__(self, dev, coarse, fine=None):
        from icpmi import prealign
        self.coarse = np.ascontiguousarray(coarse, dtype=np.float64)
        self.fine = self.coarse[:, None].copy() if fine is None else np.ascontiguousarray(fine, dtype=np.float64)
        self.fine_n = np.full(len(self.coarse), self.fine.shape[1], dtype=np.int64)
        self.max_fine = int(self.fine.shape[1])
        self.d_cs, self.d_fcs, self.d_fn = prealign.device_angle_tables(dev, self.coarse, self.fine, self.fine_n)


class Search:
    """The batched search of some cases' pairs (one voxel size), with the tables swapped per launch."""

    def __init__(self, cases, hint=0):
        from icpmi import prealign
        clouds = [c for case in cases for c in (case.src, case.tgt)]
        n = len(cases)
        self.b = prealign.RotationSearchBatch(clouds, 2 * np.arange(n), 2 * np.arange(n) + 1, cases[0].voxel, 2.0, 0.2, max_rows_hint=hint)
        assert all(case.voxel == cases[0].voxel for case in cases)
        self.b.too_many_angles = False
        self.dev = self.b.records.device

    def launch(self, coarse, fine=None):
        """-> (records, init), device copies in stream order (no synchronisation)."""
        self.b.tables = Tables(self.dev, coarse, fine)
        rec = self.b.run()
        return rec[:self.b.B].clone(), self.b.init[:self.b.B].clone()

    def direction(self):
        """The search order the prepare step chose for the targets (0..3: x, y, x + y, x - y; 4: bearing): the int32 words
        behind the row arrays of the prepared targets in the search workspace (csrc/rotsearch.hip: RsbWs)."""
        import torch
        torch.cuda.synchronize()
        raw = self.b.raw
        a256 = lambda x: (x + 255) & ~255
        at = a256(raw.total_rows * 16) + a256(raw.n_clouds * 4) + a256(raw.n_clouds * 16) + raw.total_rows * 40
        return self.b.ws[at:at + 4 * raw.n_clouds].view(torch.int32).cpu().numpy()[1::2].copy()


def _host(pairs):
    import torch
    torch.cuda.synchronize()
    return [(r.cpu().numpy(), i.cpu().numpy()) for r, i in pairs]


def _check_head(case, rec):
    pair = case.pair
    assert (int(rec[0]), int(rec[1])) == (pair.n, pair.m), (case.name, rec[:2])
    assert rec[2:4].tobytes() == pair.mu_s.tobytes() and rec[4:6].tobytes() == pair.mu_t.tobytes(), case.name


def _check_start(pair, angle, init, label):
    """R_init = [[c, -s], [s, c]] of the table entry bit for bit; t_init = mu_t - R mu_s to the rounding of its three
    operations on numbers of these magnitudes (4 u (|mu_t| + |mu_s|_1))."""
    c, s = np.cos(angle), np.sin(angle)
    assert init[:4].tobytes() == np.array([c, -s, s, c]).tobytes(), label
    LD = ref.LD
    want = [LD(pair.mu_t[0]) - (LD(c) * pair.mu_s[0] - LD(s) * pair.mu_s[1]), LD(pair.mu_t[1]) - (LD(s) * pair.mu_s[0] + LD(c) * pair.mu_s[1])]
    tol = 4 * ref.U * (np.abs(pair.mu_t).max() + np.abs(pair.mu_s).sum())
    assert abs(float(init[4] - want[0])) <= tol and abs(float(init[5] - want[1])) <= tol, (label, init[4:], want)


def _check_probe(case, p, b_last, rec, init, full, out):
    label = (case.name, round(float(np.rad2deg(p.B)), 4), p.eps, "B last" if b_last else "B first", "full" if full else "pruned")
    kB = 15 if b_last else 0
    sB, sA = float(p.sB), float(p.sA)
    out.append(f"{label} K={int(rec[K])} cscore/sB-1={rec[CSCORE] / sB - 1:.3g} tau={p.tau:.3g} evals={int(rec[EVALS])}")
    assert int(rec[STATUS]) == 0, label
    assert int(rec[K]) == kB, (label, rec[K], rec[CSCORE], sB, sA)
    assert abs(rec[CSCORE] - sB) <= p.tau * sB, (label, rec[CSCORE], sB)
    thr = ref.LD(rec[CSCORE]) * (1 - ref.LD(p.tau))
    needed = (15 if p.sA <= thr else 0) + (1 if p.sB <= thr else 0)
    assert int(rec[EVALS]) >= needed, (label, rec[EVALS], needed)
    if p.eps <= 1e-4 or full:
        assert int(rec[EVALS]) == 16, (label, rec[EVALS])
    assert int(rec[NF]) == 1 and int(rec[J]) == 0 and int(rec[FEVALS]) == 1, label
    assert rec[FSCORE].tobytes() == rec[CSCORE].tobytes(), (label, rec[FSCORE], rec[CSCORE])      # the same angle, the same sum
    _check_start(case.pair, p.B, init, label)


def _run_probes(case, libopt, projection=False, with_full=True):
    """Every probe of a case in both table orders, pruned and with RS_BATCH=full -> the log lines."""
    s = Search([case])
    kept = case.probes[0]
    assert kept
    runs = {}
    modes = (False, True) if with_full else (False,)
    for full in modes:
        libopt.setenv("ICPMI_RS_BATCH", "full") if full else (libopt.setenv("ICPMI_RS_BATCH", "projection") if projection else libopt.delenv("ICPMI_RS_BATCH"))
        runs[full] = _host([s.launch(p.table(b_last)) for p in kept for b_last in (True, False)])
    libopt.delenv("ICPMI_RS_BATCH")
    out = []
    _check_head(case, runs[False][0][0][0])
    for full in modes:
        i = 0
        for p in kept:
            for b_last in (True, False):
                rec, init = runs[full][i]
                _check_probe(case, p, b_last, rec[0], init[0], full, out)
                if full:
                    assert rec[0, :11].tobytes() == runs[False][i][0][0, :11].tobytes(), (case.name, p.B, p.eps, b_last)
                i += 1
    return s, out


@pytest.mark.parametrize("name", list(rc.cases()))
def test_the_bound_never_hides_the_winner(libopt, name):
    """Every probe of the geometry, both table orders: K names B, CSCORE is the long-double s(B) to TAU, the status is OK,
    EVALS is at least the number of entries scoring at or below CSCORE (1 - TAU) and 16 where eps <= 1e-4 (both angles'
    bounds lie 3e-4 below their scores by the kernel's own margin); and the same probes with every angle scored
    (RS_BATCH=full): record slots [:11] bit-equal."""
    _, out = _run_probes(rc.cases()[name], libopt)
    print("\n" + "\n".join(out))


def test_both_kinds_of_search_order(libopt):
    """room and walls, their copies turned by 45, 90 and 135 degrees and carried to (35, -20) m and (2e4, -3e4) m, with
    RS_BATCH=projection: the prepare step sorts the targets along each of x, y, x + y and x - y for some pair, the float32
    images are taken about the middle target row (at 2e4 m too), and the probes hold as in the order the library chooses
    (test_the_bound_never_hides_the_winner) — which is the bearing order for the scans of ``room``: both kinds are covered."""
    chosen, forced = {}, {}
    for name in ("room", "walls") + rc.FRAMES + rc.CARRIED:
        s, out = _run_probes(rc.cases()[name], libopt, projection=True, with_full=False)
        s.launch([0.0])
        chosen[name] = int(s.direction()[0])
        libopt.setenv("ICPMI_RS_BATCH", "projection")
        s.launch([0.0])
        forced[name] = int(s.direction()[0])
        libopt.delenv("ICPMI_RS_BATCH")
    print("\nsearch order, the library's choice:", chosen, "\nsearch order, projections only:", forced)
    assert set(forced.values()) == {0, 1, 2, 3}, forced
    assert chosen["room"] == 4 and all(0 <= v <= 4 for v in chosen.values()), chosen


def _groups():
    by = {}
    for case in rc.cases().values():
        if case.pair.n > 64 and case.name != "walls_2048":
            by.setdefault(case.voxel, []).append(case)
    return list(by.values())


def test_exact_ties_go_to_the_first(libopt):
    """The table [B] x 16 on every pair of more than 64 rows (so the partial-sum give-up runs: a score equal to the best
    so far must not be given up), one launch per voxel size: the same bits summed in the same order sixteen times, so
    K == 0 pins "first minimum", and EVALS == 16 (no bound exceeds the score it bounds)."""
    for B in (np.deg2rad(31.0), np.deg2rad(-90.0)):
        for group in _groups():
            s = Search(group)
            got = {}
            for full in (False, True):
                libopt.setenv("ICPMI_RS_BATCH", "full") if full else libopt.delenv("ICPMI_RS_BATCH")
                got[full] = _host([s.launch([B] * 16)])[0]
            libopt.delenv("ICPMI_RS_BATCH")
            for i, case in enumerate(group):
                rec, init = got[False][0][i], got[False][1][i]
                sB = float(case.pair.score_at(B))
                tau = case.pair.tau(sB)
                _check_head(case, rec)
                assert int(rec[STATUS]) == 0 and int(rec[K]) == 0 and int(rec[EVALS]) == 16, (case.name, rec)
                assert abs(rec[CSCORE] - sB) <= tau * sB and rec[FSCORE].tobytes() == rec[CSCORE].tobytes(), (case.name, rec[CSCORE], sB)
                _check_start(case.pair, B, init, case.name)
                assert got[True][0][i, :11].tobytes() == rec[:11].tobytes(), case.name


@pytest.mark.parametrize("name", ["walls_src65", "walls_src129"])
def test_the_fine_pass_keeps_a_near_tie(libopt, name):
    """The coarse table is [B]; its fine grid [A] x 15 + [B], and reversed; eps = 1e-9 and 1e-6 on 65 and 129 rows.  Nothing
    but the partial-sum give-up prunes here: J names B, FSCORE is s(B) to TAU, R_init / t_init are those of B's entry."""
    case = rc.cases()[name]
    s = Search([case])
    kept = [p for p in case.probes[0] if p.eps in (1e-9, 1e-6)]
    assert len(kept) >= 12
    runs = {}
    for full in (False, True):
        libopt.setenv("ICPMI_RS_BATCH", "full") if full else libopt.delenv("ICPMI_RS_BATCH")
        runs[full] = _host([s.launch([p.B], p.table(b_last)[None, :]) for p in kept for b_last in (True, False)])
    libopt.delenv("ICPMI_RS_BATCH")
    i = 0
    for p in kept:
        for b_last in (True, False):
            rec, init = runs[False][i][0][0], runs[False][i][1][0]
            label = (name, p.B, p.eps, b_last)
            sB = float(p.sB)
            assert int(rec[STATUS]) == 0 and int(rec[K]) == 0 and int(rec[NF]) == 16, label
            assert int(rec[J]) == (15 if b_last else 0), (label, rec[J], rec[FSCORE], sB, float(p.sA))
            assert abs(rec[FSCORE] - sB) <= p.tau * sB and rec[CSCORE].tobytes() == rec[FSCORE].tobytes(), (label, rec[FSCORE], sB)
            _check_start(case.pair, p.B, init, label)
            assert runs[True][i][0][0, :11].tobytes() == rec[:11].tobytes(), label
            i += 1


def _symmetric_pair():
    """A pair that a half turn about its centre maps onto itself: every cloud is its cells and their mirror images, a point
    at voxel x (cell + f) and its image at voxel x ((-1 - cell) + (1 - f)); f = 0.8 in the highest row and column, so that
    the images there are the lowest of the cloud at 0.2 (rotsearch_cases.on_cells) and every point keeps a voxel to itself."""
    def cloud(cells, phase):
        cells = np.array(cells)
        f = 0.5 + 0.2 * np.sin(np.arange(len(cells)) * phase)[:, None] * np.array([1.0, 0.6])
        for d in (0, 1):
            f[cells[:, d] == cells[:, d].max(), d] = 0.8
        return 0.125 * np.concatenate([cells + f, (-1 - cells) + (1 - f)])
    tgt = cloud([(i, j) for i in range(0, 40) for j in (0, 1)] + [(i, j) for i in (38, 39) for j in range(2, 14)], 1.7)
    src = cloud([(i, int(np.round(0.45 * i)) + j) for i in range(0, 36) for j in (0, 1)], 2.3)
    return rc.Case("half_turn", src, tgt, voxel=0.125, designed=(len(src), len(tgt)))


def test_rounding_level_near_ties(libopt):
    """A pair symmetric under a half turn: theta and theta + pi sum the same distances in another order, so the two scores
    differ by rounding at most.  The angle the search names may then be either; its long-double score may exceed the
    smallest of the table by TAU at most.  The pruned and the full run are NOT required to agree here — the record's
    bit-equality across the two holds where the table's scores differ by more than their rounding."""
    case = _symmetric_pair()
    pair = case.pair
    s = Search([case])
    for th in (0.3, -1.1, 2.0):
        table = [th + 0.02, th, th + np.pi, th - np.pi, th + 0.02 + np.pi] * 3 + [th]
        ld = np.array([pair.score_at(a) for a in table])
        assert float(abs(ld[1] - ld[2]) / ld[1]) < 1e-12, "the pair is not symmetric"
        for full in (False, True):
            libopt.setenv("ICPMI_RS_BATCH", "full") if full else libopt.delenv("ICPMI_RS_BATCH")
            rec = _host([s.launch(table)])[0][0][0]
            k = int(rec[K])
            tau = pair.tau(ld.min())
            assert int(rec[STATUS]) == 0 and 0 <= k < 16
            assert ld[k] <= ld.min() * (1 + ref.LD(tau)), (th, full, k, ld)
            assert abs(rec[CSCORE] - float(ld[k])) <= tau * float(ld[k]), (th, full, rec[CSCORE], ld[k])
    libopt.delenv("ICPMI_RS_BATCH")


def test_a_pair_above_its_capacity_hint_reports_no_winner():
    """walls with max_rows_hint = 64: ICPMI_RSB_ST_CAPACITY, the head of the record, no winner (K = 0, scores +inf, no evaluations) and
    the identity as the start."""
    case = rc.capacity_case()
    p = rc.cases()["walls"].probes[0][0]
    s = Search([case], hint=case.hint)
    rec, init = _host([s.launch(p.table(True))])[0]
    rec, init = rec[0], init[0]
    _check_head(case, rec)
    assert int(rec[STATUS]) == 2 and int(rec[K]) == 0 and int(rec[NF]) == 0 and int(rec[J]) == 0 and int(rec[EVALS]) == 0, rec
    assert np.isinf(rec[CSCORE]) and np.isinf(rec[FSCORE]) and init.tolist() == [1.0, 0.0, 0.0, 1.0, 0.0, 0.0], (rec, init)
