"""Problem.reduce_batch's reading of the library's answers, against a stub of the library (no GPU): the two passes (sizes, then
images into buffers of those sizes) and the status words the C side presets."""
import ctypes as C

import numpy as np
import pytest

N, R = 4, 2


class _StubLib:
    """sdpsr_problem_reduce_batch as a Python function: `answer(images_pass, dd, it, nb, ssq, ss, st)` fills the outputs and
    returns the call's status."""

    def __init__(self, answer):
        self.answer = answer
        self.calls = 0

    def sdpsr_problem_reduce_batch(self, ctx_h, prob_h, R_, seeds, atol, eps, pP, dd, it, nb, ssq, ss, pb, caps, st, mem):
        assert R_ == R
        self.calls += 1
        return self.answer(pb is not None, dd, it, nb, ssq, ss, st)

    def sdpsr_last_error(self, h):
        return b"stub: out of device memory"


def _problem(pkg, answer):
    class Ctx:  # the binding's own status check, on the stub
        check = pkg.Context.check
        _h = None

    ctx = Ctx()
    ctx._lib = _StubLib(answer)
    prob = object.__new__(pkg.Problem)
    prob.ctx, prob.n, prob.r, prob.atol, prob._h = ctx, N, 1, 1.5e-8, None
    return prob


def test_failure_before_the_restarts_start_raises(pkg):
    """OUT_OF_MEMORY before any restart runs: every status word still holds the library's preset SDPSR_BAD_STATE.  That is the
    call's failure, raised -- not R restarts that each report status 10."""
    def answer(images, dd, it, nb, ssq, ss, st):
        for i in range(R):
            st[i] = 10  # SDPSR_BAD_STATE, preset by the library before anything can fail
        return 8  # SDPSR_OUT_OF_MEMORY

    prob = _problem(pkg, answer)
    with pytest.raises(pkg.api.SdpsrError) as ei:
        prob.reduce_batch(R, seeds=[1, 2])
    assert ei.value.status == 8
    assert prob.ctx._lib.calls == 1


def test_images_that_did_not_fit_the_sizes_pass_are_not_returned(pkg):
    """Restart 1 fails in the sizes pass (no buffer size for its images) but reports status 0 in the images pass: its images
    were never written.  It comes back as SDPSR_BAD_STATE with blks None -- no reshape error, no zeros posing as images;
    restart 0, consistent in both passes, keeps its images."""
    d, S = 3, 5

    def answer(images, dd, it, nb, ssq, ss, st):
        for i in range(R):
            dd[i], it[i], nb[i], ss[i] = d, 2, 2, 3
            ssq[i] = S
            st[i] = 0
        if not images:
            st[1] = 2  # NumericalInconsistency: no sizes
            ssq[1] = 0
            return 2
        return 0

    prob = _problem(pkg, answer)
    res = prob.reduce_batch(R, seeds=[1, 2])
    assert prob.ctx._lib.calls == 2
    assert res[0]["status"] == 0 and res[0]["blks"].shape == (d, S)
    assert res[1]["status"] == pkg.api.BAD_STATE == 10 and res[1]["blks"] is None
    assert res[1]["P"].nparts == d


def test_loop_counters_live_in_the_measurement_library_only(pkg):
    """sdpsr_profile_loop_counts (include/sdpsr_prof.h) is exported by libsdpsr_prof.so; the product library exports no
    sdpsr_profile* symbol."""
    L = pkg._lib
    lib, prof = L.load_library(), L.load_prof_library()
    assert hasattr(prof, "sdpsr_profile_loop_counts")
    for s in L.declared_symbols(L.PROF_HEADER_PATH):
        assert s.startswith("sdpsr_profile") and not hasattr(lib, s), s
    assert np.dtype(np.uint64).itemsize == C.sizeof(C.c_uint64)
