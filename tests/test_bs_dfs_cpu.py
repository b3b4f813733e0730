"""Host runs of the depth-first output transpose (otc_bitslice.h
transpose32_bytes / _nib8 / _quad / _group8) and of the bitsliced CTR output
phase built on it (ctr_out_dfs), through the entry points beside the bitslice
self-test (csrc/cpu/bs_selftest.cpp).  The header is the code the gfx950
kernel compiles; only v_perm_b32 and the 3-input XOR are emulated."""
import ctypes

import numpy as np
import pytest

from our_tree_amd import _native

U32P = ctypes.POINTER(ctypes.c_uint32)
INTP = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def lib():
    return _native.cpu_lib()


def transpose_ref(m):
    """m[r] bit c -> out[c] bit r"""
    bits = (m[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1  # [r][c]
    return (bits.T.astype(np.uint64) << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)


def run_steps(lib, m, steps):
    a = np.ascontiguousarray(m, dtype=np.uint32).copy()
    st = (ctypes.c_int * len(steps))(*steps)
    assert lib.otc_bs_dfs_transpose(a.ctypes.data_as(U32P), st, len(steps)) == 0
    return a


def test_groups_in_any_order(lib):
    """byte stages + the four groups of 8 output words, in any order"""
    rng = np.random.default_rng(11)
    for trial in range(64):
        m = rng.integers(0, 1 << 32, 32, dtype=np.uint64).astype(np.uint32)
        order = rng.permutation(4) if trial else np.arange(4)
        got = run_steps(lib, m, [16 + int(g) for g in order])
        assert np.array_equal(got, transpose_ref(m)), (trial, order)


def test_quads_in_any_valid_order(lib):
    """the finer pieces: every 4-bit stage of a group of 8 and every quad,
    in any order that runs a group's 4-bit stage before its two quads"""
    rng = np.random.default_rng(12)
    for trial in range(64):
        m = rng.integers(0, 1 << 32, 32, dtype=np.uint64).astype(np.uint32)
        steps, pending = [], [int(g) for g in rng.permutation(4)]
        ready = []
        while pending or ready:
            if ready and (not pending or rng.integers(2)):
                steps.append(ready.pop(int(rng.integers(len(ready)))))
            else:
                g = pending.pop()
                steps.append(g)
                ready += [8 + 2 * g, 8 + 2 * g + 1]
        assert len(steps) == 4 + 8
        got = run_steps(lib, m, steps)
        assert np.array_equal(got, transpose_ref(m)), (trial, steps)


def test_a_group_yields_its_words_alone(lib):
    """finishing one group finishes exactly its 8 output words: what the
    kernel relies on when it stores a quad before the others are transposed"""
    rng = np.random.default_rng(13)
    m = rng.integers(0, 1 << 32, 32, dtype=np.uint64).astype(np.uint32)
    ref = transpose_ref(m)
    for g in range(4):
        got = run_steps(lib, m, [16 + g])
        assert np.array_equal(got[8 * g:8 * g + 8], ref[8 * g:8 * g + 8]), g
    for q in range(8):
        got = run_steps(lib, m, [q // 2, 8 + q])
        assert np.array_equal(got[4 * q:4 * q + 4], ref[4 * q:4 * q + 4]), q


def test_bad_step_rejected(lib):
    m = np.zeros(32, dtype=np.uint32)
    for bad in (-1, 4, 7, 20):
        st = (ctypes.c_int * 1)(bad)
        assert lib.otc_bs_dfs_transpose(m.ctypes.data_as(U32P), st, 1) == -1


def model(lib, planes, rk, pt, dfs, ls=8, first=10, cap=36):
    out = np.zeros(128, dtype=np.uint32)
    order = np.zeros(32, dtype=np.int32)
    rc = lib.otc_bs_ctr_out_model(planes.ctypes.data_as(U32P), rk.ctypes.data_as(U32P), pt.ctypes.data_as(U32P),
                                  out.ctypes.data_as(U32P), dfs, ls, first, cap, order.ctypes.data_as(INTP))
    return rc, out, order


@pytest.mark.parametrize("ls,first,cap", [(8, 10, 36), (8, 10, 34), (12, 14, 36), (0, 4, 40)])
def test_output_phase_model_matches_the_old_phase(lib, ls, first, cap):
    """planes in, 32 slots of ks ^ rk ^ pt out: the reordered phase gives the
    2048 blocks of a task (64 lanes x 32 slots) the old one gives, and both
    give the transposes computed independently here"""
    rng = np.random.default_rng(14)
    for lane in range(64):
        planes = rng.integers(0, 1 << 32, 128, dtype=np.uint64).astype(np.uint32)
        rk = rng.integers(0, 1 << 32, 4, dtype=np.uint64).astype(np.uint32)
        pt = rng.integers(0, 1 << 32, 128, dtype=np.uint64).astype(np.uint32)
        if lane == 0:
            pt[:] = 0  # a permuted slot shows as a wrong keystream block
        rc0, old, _ = model(lib, planes, rk, pt, 0, ls, first, cap)
        rc1, new, _ = model(lib, planes, rk, pt, 1, ls, first, cap)
        assert rc0 == 0 and rc1 == 0, (lane, rc0, rc1)
        assert np.array_equal(old, new), lane
        exp = np.stack([transpose_ref(planes[32 * w:32 * w + 32]) ^ rk[w] for w in range(4)], axis=1).reshape(-1) ^ pt
        assert np.array_equal(new, exp), lane


def test_output_phase_load_schedule(lib):
    """the default schedule: every register slot is issued once, before its
    quad is emitted and after the first emit (no load between the early ones
    and the first staged-LDS read), two quads' transposition ahead of its use, and
    the live slots (keystream not yet emitted + plaintext in registers) never
    exceed the cap of 36"""
    z = np.zeros(128, dtype=np.uint32)
    rc, _, order = model(lib, z, np.zeros(4, dtype=np.uint32), z, 1)
    assert rc == 0
    ls, first, cap = 8, 10, 36
    assert list(order[:first]) == [-1] * first
    for j in range(first, 32):
        at = int(order[j])  # slots emitted when slot j was issued
        assert at >= 4 and at % 4 == 0, (j, at)
        # a whole other quad is transposed and stored in between, and then the slot's own quad transposed
        assert 4 * (j // 4) - at >= 4, (j, at)
    for done in range(0, 33, 4):
        in_regs = [j for j in range(ls, 32) if j >= done and (j < first or order[j] <= done)]
        assert (32 - done) + len(in_regs) <= cap, (done, in_regs)


def test_unsupported_geometry(lib):
    z = np.zeros(128, dtype=np.uint32)
    rc, _, _ = model(lib, z, np.zeros(4, dtype=np.uint32), z, 1, 8, 9, 36)
    assert rc == -1
