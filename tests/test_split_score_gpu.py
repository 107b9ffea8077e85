"""evaluate()'s scoring in one device pass (``zsv_split_accuracy`` / ``train.score_splits``) against numpy, by equality.

The reference of this file is ``reference_counts``: for each class table it gathers ``pred[sel]``, ``E[chosen]`` and
``true[sel]``, takes scipy's double ``cdist`` and uses ``argsort(kind="stable")`` and ``argmin`` -- main.py:316-325 with the tie
rule made explicit.  Everything compared is an integer, so every comparison is ``==``.

One case cannot meet the "top-1 strictly between 20 % and 98 %" rule that keeps a case from passing at 0 or 100 %: with ONE row
(1, 5, 300) top-1 is 0 or 100 %.  That case is drawn so that the row misses top-1 and hits top-5 (rank 1..4): all three counters
are exercised (1, 0, 1), and the test asserts exactly that instead.
"""
import functools
import warnings
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import guarded as G
from oracle import restatement as R
from zeroshotvideoclassification_amd import _lib, synthetic

SPLITS = 10
OK, E_BAD_SHAPE, E_NULL, E_WORKSPACE = 0, 1, 2, 3

# (rows, classes, dim) -> (seed, noise) of the inputs.  The noise is set per shape so that the REFERENCE's full-set top-1 lands
# mid-range (asserted below): the signal per coordinate shrinks with 1 / sqrt(dim) and the number of competitors grows with C.
CASES = {
    (1, 5, 300): (11, 0.5),              # one row: a top-1 miss that some half-tables turn into a hit
    (37, 51, 300): (77, 0.3),
    (129, 200, 300): (77, 0.3),          # more classes than a wave, rows no multiple of 4 or 16
    (33, 17, 7): (77, 0.3),              # dim no multiple of 4
    (5, 1000, 301): (3, 0.4),
    (40, 4, 300): (77, 0.3),             # fewer than five classes, sub-tables of two
    (9, 1, 300): (77, 0.3),              # every split empty
}
UNRANGED = {(40, 4, 300), (9, 1, 300)}   # top-5 is 100 % by construction / one class: nothing to land mid-range


def eval_set(rows, classes, dim, seed, noise):
    """``synthetic.synthetic_eval_set``'s recipe; the function itself where it applies (dim 300)."""
    if dim == synthetic.EMBED_DIM:
        table, labels, true, pred = synthetic.synthetic_eval_set(rows, classes, seed=seed, noise=noise)
    else:
        g = torch.Generator().manual_seed(seed * 31 + classes)
        table = torch.nn.functional.normalize(torch.randn(classes, dim, generator=g), dim=1)
        labels = torch.randint(0, classes, (rows,), generator=g)
        true = table[labels].clone()
        pred = true * (0.5 + torch.rand(rows, 1, generator=g)) + noise * torch.randn(rows, dim, generator=g)
    return table.numpy(), labels.numpy().astype(np.int64), true.numpy(), pred.numpy()


def draw(n_classes, table_index):
    """The classes of table ``table_index`` in the order of ``class_embedding[sel_classes]`` (main.py:284-288)."""
    if table_index == 0:
        return np.arange(n_classes)
    np.random.seed(table_index - 1)
    return np.random.permutation(n_classes)[:n_classes // 2]


def positions(n_classes, splits=SPLITS):
    pos = np.full((splits + 1, n_classes), -1, dtype=np.int32)
    for t in range(splits + 1):
        chosen = draw(n_classes, t)
        pos[t][chosen] = np.arange(len(chosen))
    return pos


def cosine(a, b):
    from scipy.spatial.distance import cdist
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")                       # a zero-norm row: NaN distances, which argsort puts last
        return cdist(a, b, "cosine")


def reference_counts(pred, true, labels, table, splits=SPLITS):
    """counts (splits + 1, 3) and class_counts (C, 3) as main.py computes them, sub-tables gathered."""
    n_classes = len(table)
    counts = np.zeros((splits + 1, 3), dtype=np.int64)
    per_class = np.zeros((n_classes, 3), dtype=np.int64)
    for t in range(splits + 1):
        chosen = draw(n_classes, t)
        sel = np.ones(len(pred), dtype=bool) if t == 0 else np.isin(labels, chosen)
        if not sel.any() or len(chosen) == 0:
            continue
        order = np.argsort(cosine(pred[sel], table[chosen]), axis=1, kind="stable")
        y = cosine(true[sel], table[chosen]).argmin(1)
        top1 = order[:, 0] == y
        top5 = (order[:, :5] == y[:, None]).any(1)
        counts[t] = sel.sum(), top1.sum(), top5.sum()
        if t == 0:
            for col, hit in enumerate((np.ones_like(top1), top1, top5)):
                per_class[:, col] = np.bincount(y[hit], minlength=n_classes)
    return counts, per_class


def rule_counts(pred, true, labels, table, tie, splits=SPLITS):
    """The same counts from FULL-table distances and an explicit key: ``tie="position"`` is the rule of the entry point
    (distance, then the class's row in the gathered sub-table), ``tie="index"`` the wrong one (distance, then the original
    class index)."""
    n_classes = len(table)
    pos = positions(n_classes, splits)
    dp, dt = cosine(pred, table), cosine(true, table)
    dp, dt = np.where(np.isnan(dp), np.inf, dp), np.where(np.isnan(dt), np.inf, dt)
    counts = np.zeros((splits + 1, 3), dtype=np.int64)
    for t in range(splits + 1):
        members = np.nonzero(pos[t] >= 0)[0]
        key2 = pos[t][members] if tie == "position" else members
        for r in range(len(pred)):
            if t > 0 and not (0 <= labels[r] < n_classes and pos[t][labels[r]] >= 0):
                continue
            yi = min(range(len(members)), key=lambda i: (dt[r, members[i]], key2[i]))
            yk = (dp[r, members[yi]], key2[yi])
            rank = sum((dp[r, members[i]], key2[i]) < yk for i in range(len(members)))
            counts[t] += (1, rank == 0, rank < 5)
    return counts


@functools.lru_cache(maxsize=None)
def case(rows, classes, dim):
    seed, noise = CASES[(rows, classes, dim)]
    table, labels, true, pred = eval_set(rows, classes, dim, seed, noise)
    counts, per_class = reference_counts(pred, true, labels, table)
    for a in (table, labels, true, pred, counts, per_class):
        a.setflags(write=False)                                # shared between tests: computed once, never changed
    return table, labels, true, pred, counts, per_class


@functools.lru_cache(maxsize=None)
def tie_case():
    """Exact ties (two equal class rows, targets on them), a zero-norm prediction and a label outside the table."""
    n_classes, n = 17, 97
    table, labels, true, pred = eval_set(n, n_classes, 300, 77, 0.3)
    table = table.copy()
    table[7] = table[2]
    labels = labels.copy()
    labels[:8] = [2, 7] * 4
    true = table[labels].copy()
    pred = pred.copy()
    pred[:8] = true[:8] * 0.75 + 0.3 * pred[:8]
    pred[40] = 0.0
    labels[50] = n_classes + 3
    counts, per_class = reference_counts(pred, true, labels, table)
    for a in (table, labels, true, pred, counts, per_class):
        a.setflags(write=False)
    return table, labels, true, pred, counts, per_class


DEV = "cuda:0"


def run_abi(pred, true, labels, table, pos, per_class=False, ptrs=None, ws_short=0):
    """One raw ``zsv_split_accuracy`` call; returns (status, counts, class_counts) with the outputs on the host."""
    lib = _lib.load()
    dev = torch.device(DEV)
    rows, dim, n_classes, tables = len(pred), pred.shape[1], len(table), len(pos)
    t = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in
         dict(pred=pred, true=true, labels=labels, table=table, pos=pos).items()}
    p = {k: v.data_ptr() for k, v in t.items()}
    p.update(ptrs or {})
    counts = torch.full((tables, 3), -7, dtype=torch.int32, device=dev)         # the call zeroes them itself
    cls = torch.full((n_classes, 3), -7, dtype=torch.int32, device=dev)
    nbytes = int(lib.zsv_split_accuracy_workspace_bytes(rows, n_classes))
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    st = lib.zsv_split_accuracy(p["pred"], p["true"], p["labels"], p["table"], rows, dim, n_classes, p["pos"], tables,
                                counts.data_ptr(), cls.data_ptr() if per_class else None, ws.data_ptr(), nbytes - ws_short,
                                c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, counts.cpu().numpy().astype(np.int64), cls.cpu().numpy().astype(np.int64)


# ------------------------------------------------------------------------------------------ the reference itself (no GPU)
@pytest.mark.parametrize("rows,classes,dim", list(CASES))
def test_reference_cases_are_real_tests(rows, classes, dim):
    """A case cannot pass at 0 or 100 %: the reference's full-set top-1 lies strictly between 20 % and 98 % with top-5 above it
    (not for the two degenerate tables; the one-row case: see the module docstring).  The explicit-key restatement of the rule
    the entry point implements gives the reference's counts."""
    table, labels, true, pred, counts, per_class = case(rows, classes, dim)
    n, top1, top5 = (int(v) for v in counts[0])
    print(f"({rows}, {classes}, {dim}): full set {top1}/{n} top-1, {top5}/{n} top-5; splits {counts[1:].tolist()}")
    assert n == rows
    if rows == 1:
        assert (top1, top5) == (0, 1)
    elif (rows, classes, dim) not in UNRANGED:
        assert 0.20 * n < top1 < 0.98 * n and top5 > top1
    if (rows, classes, dim) == (9, 1, 300):
        assert not counts[1:].any()                            # C // 2 == 0: every split is empty
    if classes <= 200:                                         # (the python double loop over 1000 classes is slow, and adds nothing)
        assert np.array_equal(rule_counts(pred, true, labels, table, "position"), counts)
    assert per_class[:, 0].sum() == n and np.array_equal(per_class[:, 1:].sum(0), counts[0, 1:])


def test_tie_case_tells_the_two_tie_rules_apart():
    """Both orders of the twin classes occur among the ten draws, and breaking ties by the original class index -- the wrong
    rule -- changes the counts of at least one table."""
    table, labels, true, pred, counts, _ = tie_case()
    before = {s: int(np.nonzero(draw(17, s + 1) == 7)[0][0]) < int(np.nonzero(draw(17, s + 1) == 2)[0][0])
              for s in range(SPLITS) if 7 in draw(17, s + 1) and 2 in draw(17, s + 1)}
    assert any(before.values()) and not all(before.values()), before
    right = rule_counts(pred, true, labels, table, "position")
    wrong = rule_counts(pred, true, labels, table, "index")
    assert np.array_equal(right, counts)
    differing = np.nonzero((right != wrong).any(1))[0]
    print(f"tie case: counts {counts.tolist()}; tables that differ under index ties: {differing.tolist()}")
    assert len(differing) >= 1
    assert counts[0, 0] == 97 and (counts[1:, 0] > 0).all()


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("rows,classes,dim", list(CASES))
def test_c_abi_against_numpy(rows, classes, dim):
    table, labels, true, pred, want, _ = case(rows, classes, dim)
    st, counts, _ = run_abi(pred, true, labels, table, positions(classes))
    assert st == OK
    print(f"({rows}, {classes}, {dim}): device {counts.tolist()}\n reference {want.tolist()}")
    assert np.array_equal(counts, want)


@pytest.mark.gpu
def test_ties_zero_norm_row_and_out_of_table_label():
    table, labels, true, pred, want, want_cls = tie_case()
    st, counts, cls = run_abi(pred, true, labels, table, positions(17), per_class=True)
    assert st == OK
    wrong = rule_counts(pred, true, labels, table, "index")
    print(f"tie case: device {counts.tolist()}\n reference {want.tolist()}\n index ties {wrong.tolist()}")
    assert np.array_equal(counts, want)
    assert not np.array_equal(counts, wrong)
    assert np.array_equal(cls, want_cls)
    assert counts[0, 0] == 97                                  # the out-of-table label counts in the full set only


@pytest.mark.gpu
@pytest.mark.parametrize("rows,classes,dim", [(37, 51, 300), (129, 200, 300)])
def test_class_counts_against_numpy(rows, classes, dim):
    table, labels, true, pred, want, want_cls = case(rows, classes, dim)
    pos = positions(classes)
    st, counts, cls = run_abi(pred, true, labels, table, pos, per_class=True)
    assert st == OK
    assert np.array_equal(cls, want_cls)
    assert cls[:, 0].sum() == rows
    assert np.array_equal(cls[:, 1:].sum(0), counts[0, 1:])
    st, plain, untouched = run_abi(pred, true, labels, table, pos, per_class=False)
    assert st == OK
    assert plain.tobytes() == counts.tobytes()                 # NULL class_counts: byte-identical counts
    assert (untouched == -7).all()


def old_path_counts(pred, true, labels, table, splits=SPLITS):
    """The scoring loop ``evaluate`` ran before, rebuilt from ``train.nearest_classes``: boolean-select, gather ``E[chosen]``, two
    top-k calls per table."""
    from zeroshotvideoclassification_amd import train
    dev = torch.device(DEV)
    p, t, e = (torch.from_numpy(np.array(a)).to(dev) for a in (pred, true, table))
    counts = np.zeros((splits + 1, 3), dtype=np.int64)
    for tab in range(splits + 1):
        chosen = draw(len(table), tab)
        sel = np.ones(len(pred), dtype=bool) if tab == 0 else np.isin(labels, chosen)
        if not sel.any() or len(chosen) == 0:
            continue
        mask = torch.from_numpy(sel).to(dev)
        sub = e[torch.from_numpy(chosen).to(dev)]
        order = train.nearest_classes(p[mask], sub, 5)
        y = train.nearest_classes(t[mask], sub, 1)[:, 0]
        counts[tab] = int(sel.sum()), int((order[:, 0] == y).sum().item()), int((order == y[:, None]).any(dim=1).sum().item())
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["129x200", "ties"])
def test_full_table_distances_rank_like_gathered_sub_tables(which):
    """Against the unchanged path: the distances to the full table give the ranking bits of the gathered sub-tables."""
    from zeroshotvideoclassification_amd import train
    table, labels, true, pred, want, _ = case(129, 200, 300) if which == "129x200" else tie_case()
    old = old_path_counts(pred, true, labels, table)
    dev = torch.device(DEV)
    new = train.score_splits(*(torch.from_numpy(np.array(a)).to(dev) for a in (pred, true, labels, table)))
    assert new.is_cuda and new.dtype == torch.int32 and tuple(new.shape) == (SPLITS + 1, 3)
    print(f"{which}: old path {old.tolist()}\n one pass {new.cpu().tolist()}")
    assert np.array_equal(new.cpu().numpy(), old)
    assert np.array_equal(old, want)


def _batches(pred, labels, true, size=64):
    return [(pred[a:a + size], labels[a:a + size], true[a:a + size], None) for a in range(0, len(pred), size)]


@pytest.mark.gpu
def test_evaluate_is_one_scoring_call_and_unchanged(monkeypatch):
    from zeroshotvideoclassification_amd import train
    table, labels, true, pred = synthetic.synthetic_eval_set(150, 51, seed=7)
    want = R.evaluate_protocol(pred.numpy(), true.numpy(), labels.numpy(), table.numpy())
    lib = _lib.load()
    calls = {"zsv_split_accuracy": 0, "zsv_cosine_topk": 0}

    def counting(name):
        inner = getattr(lib, name)

        def shim(*args):
            calls[name] += 1
            return inner(*args)
        return shim

    for name in calls:
        monkeypatch.setattr(lib, name, counting(name))
    dev = torch.device(DEV)
    res = train.evaluate(torch.nn.Identity(), _batches(pred, labels, true), table, device=dev)
    assert calls == {"zsv_split_accuracy": 1, "zsv_cosine_topk": 0}, calls
    assert res == want
    assert list(res) == list(want)                             # key for key, in order
    state = np.random.get_state()
    np.random.seed(9)
    np.random.permutation(51)
    assert np.array_equal(state[1], np.random.get_state()[1]) and state[2] == np.random.get_state()[2]

    per = train.evaluate(torch.nn.Identity(), _batches(pred, labels, true), table, device=dev, per_class=True)
    assert calls["zsv_split_accuracy"] == 2 and calls["zsv_cosine_topk"] == 0
    assert set(per) - set(res) == {"class_counts", "mean_class_accuracy"}
    assert {k: per[k] for k in res} == res
    _, want_cls = reference_counts(pred.numpy(), true.numpy(), labels.numpy(), table.numpy(), splits=0)
    assert np.array_equal(per["class_counts"], want_cls)
    seen = want_cls[:, 0] > 0
    assert per["mean_class_accuracy"] == float(np.mean(want_cls[seen, 1] / want_cls[seen, 0] * 100))

    # score_splits: the device tensors, and compute_accuracy on top of it
    args = [a.to(dev) for a in (pred, true, labels, table)]
    counts, cls = train.score_splits(*args, per_class=True)
    assert counts.is_cuda and cls.is_cuda and tuple(counts.shape) == (11, 3) and tuple(cls.shape) == (51, 3)
    assert np.array_equal(cls.cpu().numpy(), want_cls)
    assert train.compute_accuracy(args[0], args[3], args[1]) == (want["accuracy"], want["accuracy_top5"])
    empty = train.score_splits(args[0][:0], args[1][:0], args[2][:0], args[3])
    assert empty.is_cuda and tuple(empty.shape) == (11, 3) and not empty.any().item()
    assert calls["zsv_cosine_topk"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("rows,classes,dim", [(37, 51, 300), (33, 17, 7)])
def test_memory_contract(rows, classes, dim):
    """Workspace of exactly the queried size and outputs of exactly their shapes between guard bands: both prefills give the
    same bytes and the bands stay intact; inputs of exactly their extent between poisoned bands: the counts do not move."""
    table, labels, true, pred, want, want_cls = case(rows, classes, dim)
    lib = _lib.load()
    dev = torch.device(DEV)
    pos = positions(classes)
    tables = len(pos)
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    nbytes = int(lib.zsv_split_accuracy_workspace_bytes(rows, classes))
    ins = dict(pred=pred, true=true, labels=labels, table=table, pos=pos)
    plain = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in ins.items()}

    def call(p, counts, cls, ws):
        st = lib.zsv_split_accuracy(p["pred"], p["true"], p["labels"], p["table"], rows, dim, classes, p["pos"], tables,
                                    counts.ptr, cls.ptr, ws.ptr, nbytes, stream)
        torch.cuda.synchronize()
        assert st == OK
        for name, buf in (("counts", counts), ("class_counts", cls), ("workspace", ws)):
            buf.check(f"zsv_split_accuracy {name}")
        return counts.bytes().cpu(), cls.bytes().cpu()

    seen = []
    for fill in G.FILLS:                                       # outputs and workspace: exact extents, two prefills
        counts = G.guarded_like(torch.int32, (tables, 3), dev, fill)
        cls = G.guarded_like(torch.int32, (classes, 3), dev, fill)
        ws = G.guarded(nbytes, dev, fill)
        seen.append(call({k: v.data_ptr() for k, v in plain.items()}, counts, cls, ws))
    assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1])
    assert np.array_equal(seen[0][0].numpy().view(np.int32).reshape(tables, 3), want)
    assert np.array_equal(seen[0][1].numpy().view(np.int32).reshape(classes, 3), want_cls)

    for band in G.BAND_BYTES:                                  # inputs: exact extents, two poisons around them
        held = {k: G.guarded_copy(v, dev, guard_byte=band) for k, v in plain.items()}
        counts = G.guarded_like(torch.int32, (tables, 3), dev, 0xFF)
        cls = G.guarded_like(torch.int32, (classes, 3), dev, 0xFF)
        ws = G.guarded(nbytes, dev, 0xFF)
        got = call({k: v.ptr for k, v in held.items()}, counts, cls, ws)
        for name, buf in held.items():
            buf.check(f"zsv_split_accuracy input {name}")
        assert torch.equal(got[0], seen[0][0]) and torch.equal(got[1], seen[0][1]), f"band 0x{band:02X}"


@pytest.mark.gpu
def test_error_codes_without_a_launch():
    table, labels, true, pred, want, _ = case(37, 51, 300)
    pos = positions(51)
    st, counts, _ = run_abi(pred, true, labels, table, pos, ws_short=8)
    assert st == E_WORKSPACE and (counts == -7).all()          # not even zeroed: nothing ran
    st, counts, _ = run_abi(pred, true, labels, table, pos, ptrs={"labels": None})
    assert st == E_NULL and (counts == -7).all()
    st, counts, _ = run_abi(pred, true, labels, table, pos[:1], ptrs={"labels": None})
    assert st == OK and np.array_equal(counts, want[:1])       # the whole table alone does not consult the labels
