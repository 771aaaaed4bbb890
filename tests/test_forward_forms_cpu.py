"""CPU: the case table of tests/forward_forms_cases.py against the library's own dispatch ladders (the elo_*_form queries of
include/elo.h read the argument block only: no GPU, fake addresses of the case's alignment), every form covered, the fp16 refusals,
and the pool error constants of tests/forward_forms_bounds.py against float32 restatements of each form's arithmetic."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import forward_forms_bounds as bounds
import forward_forms_cases as table
from conftest import ROOT, load_pkg
from forms_inputs import pool_forward_inputs

QUERY = {"encode1": "elo_cv_encode1_form", "encode2": "elo_cv_encode2_form", "pool": "elo_masked_softmax_pool_form"}
ENUM = {"encode1": "ELO_ENCODE1_", "encode2": "ELO_ENCODE2_", "pool": "ELO_POOL_"}
# forms that fp16 storage never takes (include/elo.h): it has no scalar kernels, and the wave-per-point pool is fp32 only
F32_ONLY = {"encode1": {"scalar"}, "encode2": {"scalar"}, "pool": {"scalar", "wave1", "wave2", "wave4", "wave8"}}
BASE = 0x7f0000000000                                    # fake device addresses, 4 KB apart and 4 KB aligned: never dereferenced


def fake_args(case):
    """The argument block a call of `case` would pass, with fake non-null addresses of the case's alignment."""
    L = load_pkg("_lib")
    esz = 2 if case.dtype == "f16" else 4
    code = L.ELO_F16 if case.dtype == "f16" else L.ELO_F32
    p = [BASE + 4096 * i for i in range(8)]
    if case.op == "encode1":
        return L.CvEncode1Args(case.B, case.N, case.K, case.H, case.W, case.C, p[0], p[1] + case.offset, p[2], p[3] + case.offset,
                               p[4], p[5], p[6], code)
    if case.op == "encode2":
        return L.CvEncode2Args(case.B, case.N, case.K, case.H, case.W, case.C, case.Cc, p[0], p[1] + case.offset, p[2] + case.offset,
                               p[3], p[4], p[5], p[6], code)
    width, first = case.wide or (case.C, 0)
    return L.SoftmaxPoolArgs(case.B, case.N, case.K, case.C, p[0], p[1] + first * esz + case.offset, width, p[2], p[3], code)


def ask(case):
    """The form's name, or the negative status."""
    L, tuning = load_pkg("_lib"), load_pkg("tuning")
    names = {"encode1": L.ENCODE1_FORMS, "encode2": L.ENCODE2_FORMS, "pool": L.POOL_FORMS}[case.op]
    with tuning.override(**dict(case.tuning or ())):
        rc = getattr(L.lib(), QUERY[case.op])(ctypes.byref(fake_args(case)))
    return names[rc] if rc >= 0 else rc


def header_forms(op):
    header = open(os.path.join(ROOT, "include", "elo.h")).read()
    found = re.findall(r"\b%s([A-Z0-9]+)\s*=\s*(\d+)" % ENUM[op], header)
    return [name.lower() for name, _ in sorted(found, key=lambda nv: int(nv[1]))]


@pytest.mark.parametrize("case", table.CASES, ids=table.case_id)
def test_case_reaches_the_form_it_names(case):
    assert ask(case) == case.form


@pytest.mark.parametrize("rows,C,offset,form", table.ENCODE1_THRESHOLDS)
def test_cv_encode1_row_thresholds(rows, C, offset, form):
    assert ask(table.Case("encode1", "f32", 1, rows, 8, 29, 1, C, None, None, offset, None, form)) == form


@pytest.mark.parametrize("op", ["encode1", "encode2", "pool"])
def test_every_form_of_the_library_has_a_case(op):
    """The enumerators of include/elo.h are the forms; the binding names them in the same order; and every form a storage type can
    reach has a case in that storage type.  A form added to the library without a case fails here."""
    L = load_pkg("_lib")
    forms = header_forms(op)
    assert forms and tuple(forms) == {"encode1": L.ENCODE1_FORMS, "encode2": L.ENCODE2_FORMS, "pool": L.POOL_FORMS}[op]
    for dtype in ("f32", "f16"):
        reachable = set(forms) - (F32_ONLY[op] if dtype == "f16" else set())
        covered = {c.form for c in table.CASES if c.op == op and c.dtype == dtype}
        assert covered == reachable, (dtype, sorted(reachable - covered), sorted(covered - reachable))


def test_pool_cases_cover_the_slice_variant():
    """every vec / wave case of the pool also runs with its values a channel slice of a wider tensor"""
    pool = [c for c in table.CASES if c.op == "pool" and c.form != "scalar" and not c.offset]
    plain = {c for c in pool if c.wide is None}
    assert plain and {c._replace(wide=None) for c in pool if c.wide} == plain


def test_cases_have_a_tail():
    """No encode case's row count is a multiple of its form's workgroup span, K does not divide the span (a workgroup begins
    mid-centre), and the B = 2 cases put the batch boundary inside a workgroup; the pool's point count is no multiple of 4."""
    for c in table.CASES:
        if c.op == "pool":
            assert (c.B * c.N) % 4
            continue
        s = table.span(c)
        assert table.rows(c) % s and s % c.K, (c, s)
        if c.B > 1:
            assert (c.N * c.K) % s, (c, s)


@pytest.mark.parametrize("refusal", table.REFUSALS, ids=lambda r: r.why.replace(" ", "_"))
def test_fp16_refusals(refusal):
    L = load_pkg("_lib")
    assert ask(refusal.case) == -1                       # ELO_ERR_ARG
    assert b"fp16 needs" in L.lib().elo_last_error()
    assert isinstance(ask(refusal.case._replace(dtype="f32")), str)                             # (fp32 takes the same block)


def test_queries_validate_like_the_entry_points():
    L = load_pkg("_lib")
    lib = L.lib()
    assert lib.elo_cv_encode1_form(None) == -1 and b"elo_cv_encode1_form: null argument block" in lib.elo_last_error()
    a = fake_args(table.ENCODE1[0])
    a.feat2 = None
    assert lib.elo_cv_encode1_form(ctypes.byref(a)) == -1 and b"null tensor pointer" in lib.elo_last_error()
    a = fake_args(table.ENCODE2[0])
    a.npoints += 1
    assert lib.elo_cv_encode2_form(ctypes.byref(a)) == -1 and b"H*W" in lib.elo_last_error()
    a = fake_args(table.POOL[0])
    a.values_stride = a.C - 1
    assert lib.elo_masked_softmax_pool_form(ctypes.byref(a)) == -1 and b"bad sizes" in lib.elo_last_error()
    a = fake_args(table.POOL[0])
    a.dtype = 7
    assert lib.elo_masked_softmax_pool_form(ctypes.byref(a)) == -1 and b"dtype" in lib.elo_last_error()
    with pytest.raises(L.EloError):
        L.form("elo_cv_encode1_form", fake_args(table.REFUSALS[0].case))


# one restatement per (form's arithmetic, K, C): the slice / offset / tuning variants of a case compute the same numbers
_POOL_ARITH = sorted({(c.form, c.dtype, c.K, c.C) for c in table.CASES if c.op == "pool"})


@pytest.mark.parametrize("form,dtype,K,C", _POOL_ARITH, ids=lambda v: str(v))
def test_pool_constants_hold_for_a_float32_restatement(form, dtype, K, C):
    """tests/forward_forms_bounds.py derives the constant in front of UNIT from each form's operation count.  Before the GPU test
    trusts it: the form's arithmetic restated in float32 numpy, on the GPU test's inputs, stays within HALF of it."""
    rng = np.random.default_rng(K * 100 + C)
    lg, v, m = pool_forward_inputs(rng, 2, 301, K, C, f16=dtype == "f16")
    got = bounds.pool_restatement(form)(lg, v, m)
    ref, unit, scale = bounds.pool_reference(*(torch.from_numpy(a).double() for a in (lg, v, m)))
    err = (torch.from_numpy(got).double() - ref).abs()
    assert bool(torch.isfinite(err).all())
    ratio = float(((err - K * bounds.POOL_ABS * scale).clamp(min=0) / unit).max())
    print("restatement %s K=%d C=%d: worst error %.2f UNIT of a constant of %d" % (form, K, C, ratio, bounds.pool_constant(form, K)))
    assert ratio <= bounds.pool_constant(form, K) / 2
    mean = torch.from_numpy(v).double().mean(2)[:, 0]                 # point 0 of every batch element is all masked
    assert bool(((torch.from_numpy(got).double()[:, 0] - mean).abs() <= bounds.pool_constant(form, K) / 2 * unit[:, 0]).all())
