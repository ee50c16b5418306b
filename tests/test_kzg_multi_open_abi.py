"""CPU: the multi-opening entry point (include/mzk.h against lib.py, by arity; exported by the built library), the FFT-size rules of
pcs/mod.rs:259-322 as the Python layer restates them, and the refusals UnivariateKzgPCS.multi_open_rou* make before anything touches the GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, ARITY = "mzk_kzg_multi_open_rou_dev", 9


def test_the_entry_point_is_declared_bound_and_exported(mj):
    from importlib import import_module
    lib = import_module("mpc-jellyfish_amd.lib")
    text = open(os.path.join(ROOT, "include", "mzk.h")).read()
    m = re.search(r"MZK_API\s+int32_t\s+%s\s*\(([^;]*)\);" % NAME, text)
    assert m, NAME + " is not declared in include/mzk.h"
    assert len(m.group(1).split(",")) == ARITY == len(lib._SIGS[NAME])
    assert hasattr(mj.load(), NAME), NAME + " is not exported"
    assert NAME in lib.EXPORTS
    assert "trailing zero coefficients are not trimmed" in text and "above 21" in text      # the contract states the degree rule and the cap


def _is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def _next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def _fft_size(degree):
    """pcs/mod.rs:310-322: twice a power of two, else the next power of two (usize::next_power_of_two(0) = 1)"""
    return 2 * degree if _is_pow2(degree) else _next_pow2(degree)


DEGREES = (0, 1, 2, 3, 14, 15, 16, 17, 18)


def test_fft_sizes_follow_the_reference(mj):
    assert [_fft_size(d) for d in DEGREES] == [1, 2, 4, 4, 16, 16, 32, 32, 32]
    for degree in DEGREES:
        assert mj.checked_fft_size(degree) == mj.kzg.checked_fft_size(degree) == _fft_size(degree), degree
        for num_points in (1, 5, 29, 33):
            want = _next_pow2(max(_fft_size(degree) + 1, num_points))      # pcs/mod.rs:264-267, then Radix2EvaluationDomain::new rounds up
            for c in (mj.params.BLS12_381, mj.params.BN254):
                dom = mj.UnivariateKzgPCS.multi_open_rou_eval_domain(c, degree, num_points)
                assert dom.size == want and dom.coset_offset_is_one() and dom.curve is c, (degree, num_points)
    with pytest.raises(mj.PCSError):
        mj.checked_fft_size(1 << 63)                                       # usize overflow
    with pytest.raises(mj.PCSError):
        mj.UnivariateKzgPCS.multi_open_rou_eval_domain(mj.params.BN254, 1 << 28, 1)        # past the two-adicity of Fr


def test_refusals_come_before_the_library_is_loaded(mj, monkeypatch):
    from importlib import import_module
    lib = import_module("mpc-jellyfish_amd.lib")

    def no_device(*a, **k):
        raise AssertionError("the refusal comes first: the library was asked for")
    monkeypatch.setattr(lib, "ensure_init", no_device)
    monkeypatch.setattr(lib, "load", no_device)
    K = mj.UnivariateKzgPCS
    c = mj.params.BLS12_381
    dom = mj.Radix2EvaluationDomain(c, 4)
    pp = mj.UnivariateProverParam(c, 0, 17)                                # (a handle that is never used)
    poly = lambda n: np.zeros((n, 4), dtype=np.uint64)
    coset = dom.get_coset(c.fr_generator)
    with pytest.raises(mj.PCSError, match="coset"):
        K.multi_open_rou_evals(poly(5), 4, coset)
    for call in (lambda d: K.multi_open_rou(pp, poly(5), 4, d), lambda d: K.multi_open_rou_proofs(pp, poly(5), 4, d)):
        with pytest.raises(mj.PCSError, match="coset"):
            call(coset)
        with pytest.raises(mj.PCSError, match="coset"):
            call(mj.Radix2EvaluationDomain(mj.params.BN254, 4))           # the other curve's field
    # len = 17 > N = 16: the evaluations are refused, and multi_open_rou with them (its evaluation step runs first) ...
    with pytest.raises(mj.PCSError, match="17 num_of_coeffs"):
        K.multi_open_rou_evals(poly(17), 16, dom)
    with pytest.raises(mj.PCSError, match="17 num_of_coeffs"):
        K.multi_open_rou(pp, poly(17), 16, dom)
    # ... d = 32 > N = 16: the proofs are
    with pytest.raises(mj.PCSError, match="32 num_of_coeffs"):
        K.multi_open_rou_proofs(mj.UnivariateProverParam(c, 0, 64), poly(18), 16, dom)
    # fewer than d points: a view of 15 points under len = 17 (d = 16)
    short = mj.UnivariateProverParam(c, 0, 15, offset=2, owner=False)
    with pytest.raises(mj.PCSError, match="holds 15 points"):
        K.multi_open_rou_proofs(short, poly(17), 16, mj.Radix2EvaluationDomain(c, 5))
    with pytest.raises(mj.PCSError, match="holds 15 points"):
        K.multi_open_rou(short, poly(17), 16, mj.Radix2EvaluationDomain(c, 5))
    # trim_fft_size: checked_fft_size(9) = 16 points past the first
    assert K.trim_fft_size(pp, 9).length == 17 and K.trim_fft_size(pp, 8).length == 17 and K.trim_fft_size(pp, 7).length == 9
    with pytest.raises(mj.PCSError, match="Requesting degree of 32 for FFT"):
        K.trim_fft_size(pp, 16)
