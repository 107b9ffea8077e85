"""Host side of evaluate()'s one-pass scoring (``zsv_split_accuracy``; no GPU needed): the C ABI is declared, exported and
bound; bad arguments are refused before any launch; ``train.split_tables`` inverts the reference's own draw
(main.py:284-285) and leaves numpy's global generator where the reference leaves it; no CPU fallback."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from zeroshotvideoclassification_amd import _lib, synthetic, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_BAD_SHAPE, E_NULL, E_WORKSPACE, E_TOO_LARGE = 0, 1, 2, 3, 4


def test_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "zsv_hip.h")).read()
    P, i32 = ctypes.c_void_p, ctypes.c_int32
    want = {"zsv_split_accuracy_workspace_bytes": (ctypes.c_size_t, [i32, i32]),
            "zsv_split_accuracy": (ctypes.c_int, [P, P, P, P, i32, i32, i32, P, i32, P, P, P, ctypes.c_size_t, P])}
    for name, (res, args) in want.items():
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/zsv_hip.h"
        assert _lib.SIGNATURES[name] == (res, args)
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args
    # the header's prototype has as many parameters as the binding, pointers where the binding has pointers
    proto = re.search(r"int zsv_split_accuracy\((.*?)\);", header, re.S).group(1)
    params = [p.strip() for p in proto.split(",")]
    assert len(params) == len(want["zsv_split_accuracy"][1])
    assert [("*" in p) for p in params] == [a is P for a in want["zsv_split_accuracy"][1]]
    assert "main.py:281-304" in header and "main.py:316-325" in header          # the reference call sites, like every entry point


def test_workspace_is_two_distance_matrices_at_the_class_pitch():
    lib = _lib.load()
    for rows, classes in ((1, 5), (37, 51), (129, 200), (5, 1000), (16, 16)):
        pitch = (classes + 15) // 16 * 16
        assert lib.zsv_split_accuracy_workspace_bytes(rows, classes) == 2 * rows * pitch * 8
        assert lib.zsv_split_accuracy_workspace_bytes(rows, classes) == 2 * lib.zsv_cosine_topk_workspace_bytes(rows, classes)
    assert lib.zsv_split_accuracy_workspace_bytes(0, 5) == 0 and lib.zsv_split_accuracy_workspace_bytes(5, 0) == 0


def test_bad_arguments_are_refused_before_any_launch():
    """No device is needed (or touched): every refusal below returns before the first HIP call.  The pointers are never
    dereferenced on the host; any non-NULL value stands for one."""
    lib = _lib.load()
    p = 0x1000
    big = 1 << 40

    def call(pred=p, true=p, labels=p, table=p, rows=8, dim=300, classes=11, pos=p, tables=11, counts=p, per_class=None, ws=p,
             nbytes=big):
        return lib.zsv_split_accuracy(pred, true, labels, table, rows, dim, classes, pos, tables, counts, per_class, ws, nbytes, None)

    for name in ("pred", "true", "table", "pos", "counts", "ws"):
        assert call(**{name: None}) == E_NULL, name
    assert call(labels=None) == E_NULL                                  # the splits consult the labels ...
    for name in ("rows", "dim", "classes", "tables"):
        for bad in (0, -3):
            assert call(**{name: bad}) == E_BAD_SHAPE, (name, bad)
    assert call(labels=None, tables=1, rows=0) == E_BAD_SHAPE           # ... the whole table alone does not: NULL is no error there
    assert call(rows=1 << 24, dim=300) == E_TOO_LARGE                   # rows * dim >= 2^31, zsv_cosine_topk's bound
    assert call(classes=1 << 24, dim=300) == E_TOO_LARGE
    assert call(tables=2049) == E_TOO_LARGE
    need = lib.zsv_split_accuracy_workspace_bytes(8, 11)
    assert call(nbytes=need - 8) == E_WORKSPACE
    assert call(nbytes=0) == E_WORKSPACE


@pytest.mark.parametrize("n_classes", [1, 4, 17, 101])
def test_split_tables_invert_the_reference_draw(n_classes):
    pos = train.split_tables(n_classes, 10)
    assert pos.shape == (11, n_classes) and pos.dtype == np.int32
    assert np.array_equal(pos[0], np.arange(n_classes))
    for split in range(10):
        np.random.seed(split)                                                       # main.py:284-285
        chosen = np.random.permutation(n_classes)[:n_classes // 2]
        row = pos[split + 1]
        assert int((row >= 0).sum()) == n_classes // 2
        assert np.array_equal(row[chosen], np.arange(len(chosen)))                  # pos[s + 1][chosen[j]] == j
        assert np.all(row[np.setdiff1d(np.arange(n_classes), chosen)] == -1)
    if n_classes == 1:
        assert np.all(pos[1:] == -1)                                                # C // 2 == 0: every split is empty
    assert train.split_tables(n_classes, 0).shape == (1, n_classes)


@pytest.mark.parametrize("n_classes", [1, 4, 17, 101])
def test_split_tables_leave_numpy_where_the_reference_leaves_it(n_classes):
    np.random.seed(9)
    np.random.permutation(n_classes)
    want = np.random.get_state()
    np.random.seed(12345)
    train.split_tables(n_classes, 10)
    got = np.random.get_state()
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2:] == want[2:]
    first = train.split_tables(n_classes, 10)
    np.random.seed(777)                                                             # a second call replays the draws: nothing is cached
    assert np.array_equal(train.split_tables(n_classes, 10), first)
    got = np.random.get_state()
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2:] == want[2:]
    state = np.random.get_state()
    train.split_tables(n_classes, 0)                                                # no splits: no draws (compute_accuracy)
    after = np.random.get_state()
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:]


def test_no_cpu_fallback():
    table, labels, true, pred = synthetic.synthetic_eval_set(8, 11)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.score_splits(pred, true, labels, table)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.score_splits(pred, true, labels, table, splits=0, per_class=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.compute_accuracy(pred, table, true)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.evaluate(torch.nn.Identity(), [(pred, labels, true, None)], table, device=torch.device("cpu"))
