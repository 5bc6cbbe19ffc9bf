"""No form outlives its call.

What kind of call a multiply enqueues -- two-phase, through, speculated, a reuse sequence with or without its scan, the
stage entry point -- is an argument of the functions that enqueue it (speck_amd/csrc/pipeline.hip, CallForm), built by
the call and gone with it.  ONE config serves two problems through every form in turn, each call right behind a call of
ANOTHER form: the placement of a reuse sequence, the staged row offsets, the gate of a through call, the numeric-first
window of the other problem -- nothing of the call before may show in the call after.  Every result is the oracle's
(row_offsets and col_ids bit-exact, values within 1e-12 * sum|a*b|), and the path every call took is the one the
sequence took before the form was an argument.
"""
import ctypes as C_

import numpy as np
import pytest

import speck_amd as sa
from speck_amd import _lib
from oracle import pyoracle as po
from test_gpu_parity import _assert_matches_oracle, _hostile_b, to_po, to_sa
from test_gpu_through import _scribble

pytestmark = pytest.mark.gpu

FLAGS = ("replayed", "pred_stages", "eager_through", "eager_speculated", "nf_direct", "esc_fused")


def _flags(cfg):
    st = cfg.last_stats()
    return tuple(int(st[k]) for k in FLAGS)


def call_form_sequence():
    """The steps of the test, one at a time: (name, flags of last_stats() behind the step)."""
    X = to_po(sa.gen_matrix("mac_econ", 0.08, 3, signed=True))    # register-class, hash and numeric-first rows
    Y = to_po(sa.gen_matrix("webbase", 0.04, 7, signed=True))     # ... and the heavy classes
    L = _lib.load()
    cfg = sa.spECKConfig.initialize(0)
    try:
        dX, dXb, dY = sa.dCSR.from_host(to_sa(X)), sa.dCSR.from_host(to_sa(X)), sa.dCSR.from_host(to_sa(Y))
        dC, dCy = sa.dCSR(), sa.dCSR()

        def multiply_x(name):
            sa.MultiplyspECK(dX, dXb, dC, cfg)
            _assert_matches_oracle(dC, X, X)
            return name, _flags(cfg)

        # (reuse is on by default, and the second identical call would already be a reuse sequence: it is on for step 3
        #  alone.  A reuse sequence writes C before the verdict on B is in -- step 7 wants C untouched.)
        cfg.set_option("reuse", 0)
        yield multiply_x("1 two-phase")
        yield multiply_x("2 through")
        cfg.set_option("reuse", 1)
        yield multiply_x("3a through")
        yield multiply_x("3b plan made, replayed")
        yield multiply_x("3c replayed without a scan")
        cfg.set_option("reuse", 0)
        sa.MultiplyspECK(dY, dY, dCy, cfg)
        _assert_matches_oracle(dCy, Y, Y)
        yield "4 other problem", _flags(cfg)
        ro, nnz = sa.symbolic(dY, dY, cfg)
        Ry, _ = po.spgemm(Y, Y)
        assert nnz == Ry.nnz and (ro == Ry.row_offsets).all()
        yield "5 symbolic", _flags(cfg)                            # (the stage entry point publishes nothing: step 4's)
        yield multiply_x("6 first problem again")
        # B's rows shuffled under the same pointers: the unsorted error, and nothing of C written
        _scribble(dC)
        before = dC.to_host()
        bad = np.ascontiguousarray(_hostile_b(X, "shuffled", np.random.default_rng(5)).col_ids)
        assert L.speck_dcsr_update(C_.byref(dXb._c), None, bad.ctypes.data, None, 8) == 0
        with pytest.raises(sa.SpeckError) as e:
            sa.MultiplyspECK(dX, dXb, dC, cfg)
        assert e.value.status == 8
        after = dC.to_host()
        assert after.nnz == before.nnz and (after.row_offsets == before.row_offsets).all()
        assert (after.col_ids == before.col_ids).all()
        assert after.data.tobytes() == before.data.tobytes()
        assert L.speck_dcsr_update(C_.byref(dXb._c), None, np.ascontiguousarray(X.col_ids).ctypes.data, None, 8) == 0
        yield multiply_x("8 B restored")
    finally:
        cfg.cleanup()


# Recorded by running call_form_sequence() on the PARENT of the commit that made the form an argument (twice: the same
# flags both times), not on the code under test.
#            replayed pred_stages eager_through eager_speculated nf_direct esc_fused
EXPECTED = {
    "1 two-phase": (0, 0, 0, 0, 0, 0),
    "2 through": (0, 0, 1, 1, 0, 0),
    "3a through": (0, 0, 1, 1, 0, 0),
    "3b plan made, replayed": (1, 7, 0, 0, 1, 1),
    "3c replayed without a scan": (1, 15, 0, 0, 1, 1),
    "4 other problem": (0, 0, 0, 0, 0, 0),
    "5 symbolic": (0, 0, 0, 0, 0, 0),
    "6 first problem again": (0, 0, 0, 0, 0, 0),
    "8 B restored": (0, 0, 1, 1, 0, 0),
}


def test_no_form_outlives_its_call():
    seen = dict(call_form_sequence())
    for name, flags in seen.items():
        print(name, dict(zip(FLAGS, flags)))
    assert seen == EXPECTED
