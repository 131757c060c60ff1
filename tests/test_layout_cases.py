"""CPU checks of the layout matrix (tests/layout_cases.py, run on the GPU by
test_gpu_layouts.py): the guard arena reports a stray byte in every kind of
guard region, and the case tables reach every kernel name and both sides of
every clause of the dispatch predicates (tests/test_dispatch.py)."""
import numpy as np
import pytest

import ecc_amd as E
import layout_cases as L


# ---------------------------------------------------------------- the arena
def _arena():
    A = L.Arena(seed=11)
    a_in = A.add("input", 1000, off=1)
    a_out = A.add("rows", 5 * 96, off=8)  # 5 rows of 64 used bytes, pitch 96
    A.build()
    A.allow_rows(a_out, 5, 96, 64)
    return A, a_in, a_out


def test_arena_geometry():
    A, a_in, a_out = _arena()
    assert a_in % 256 == 1 and a_out % 256 == 8
    assert a_in >= L.GUARD and a_out >= a_in + 1000 + L.GUARD and A.size >= a_out + 5 * 96 + L.GUARD
    assert A.size % 256 == 0 and A.host.shape == (A.size,) == A.mask.shape
    # noise, not a constant fill: no byte value dominates
    assert np.bincount(A.host, minlength=256).max() < A.size // 16
    assert A.mask.sum() == 5 * 64


def test_arena_accepts_allowed_writes():
    A, _, a_out = _arena()
    got = A.host.copy()
    for r in range(5):
        got[a_out + r * 96: a_out + r * 96 + 64] ^= 0xFF
    assert A.violations(got) == []
    assert A.violations(A.host.copy()) == []


@pytest.mark.parametrize("what,pos", [
    ("first byte before a base", lambda a_in, a_out, A: a_out - 1),
    ("256 bytes before a base", lambda a_in, a_out, A: a_out - L.GUARD),
    ("first byte after the last row", lambda a_in, a_out, A: a_out + 4 * 96 + 64),
    ("last byte of the guard after the end", lambda a_in, a_out, A: a_out + 5 * 96 + L.GUARD - 1),
    ("row padding, first byte", lambda a_in, a_out, A: a_out + 64),
    ("row padding, last byte", lambda a_in, a_out, A: a_out + 2 * 96 - 1),
    ("input buffer, first byte", lambda a_in, a_out, A: a_in),
    ("input buffer, last byte", lambda a_in, a_out, A: a_in + 999),
    ("guard before the first buffer", lambda a_in, a_out, A: 0),
    ("last byte of the arena", lambda a_in, a_out, A: A.size - 1),
])
def test_arena_reports_one_stray_byte(what, pos):
    A, a_in, a_out = _arena()
    p = pos(a_in, a_out, A)
    assert not A.mask[p], what
    got = A.host.copy()
    got[p] ^= 1  # one bit of one byte
    bad = A.violations(got)
    assert len(bad) == 1, (what, bad)
    # and writing the byte that was there is no violation (nothing to see)
    assert A.violations(A.host.copy()) == []


def test_arena_names_the_region():
    A, a_in, a_out = _arena()
    got = A.host.copy()
    got[a_out + 64] ^= 1
    got[a_in + 5] ^= 1
    got[a_out - 3] ^= 1
    assert A.violations(got) == ["input+5 (of 1000)", "rows-3 (of 480)", "rows+64 (of 480)"]
    got[:] ^= 1
    assert len(A.violations(got, limit=4)) == 5  # truncated with "..."


# ---------------------------------------------------------------- coverage of the tables
def _enc_facts():
    for shape, var in L.enc_cases():
        _, k, _ = E.code_params(shape.nv)
        pay, ps, sh, ss = L.enc_layout(shape, var, E.shard_len(shape.nv, shape.plen))
        yield dict(name=getattr(shape, var.cls), k=k, batch=var.batch, pay=pay, ps=ps, sh=sh, ss=ss,
                   pieces=E.shard_len(shape.nv, shape.plen) // 2)


def _rec_facts():
    for shape, var in L.rec_cases():
        n, k, _ = E.code_params(shape.nv)
        sl = E.shard_len(shape.nv, shape.plen)
        sh, ss, pr, el, out, os_ = L.rec_layout(shape, var, sl, k)
        yield dict(name=getattr(shape, var.cls), n=n, k=k, batch=var.batch, sh=sh, ss=ss, pr=pr, el=el,
                   out=out, os=os_, cols=sl // 2)


def test_every_kernel_has_a_gpu_case():
    named = {f["name"] for f in _enc_facts()} | {f["name"] for f in _rec_facts()}
    assert named == set(L.KERNELS)


# each clause of the dispatch predicates as a function of a case's layout:
# True / False = the side the case is on, None = the clause does not bear on it
ENC_CLAUSES = {
    "payload base mod 16": lambda f: f["pay"] % 16 == 0,
    "shard base mod 8": lambda f: f["sh"] % 8 == 0,
    "shard base mod 2": lambda f: f["sh"] % 2 == 0,
    "pstride mod 16 (batch > 1)": lambda f: f["ps"] % 16 == 0 if f["batch"] > 1 else None,
    "batch == 1 with pstride off 16": lambda f: f["batch"] == 1 if f["ps"] % 16 else None,
    "sstride mod 8": lambda f: f["ss"] % 8 == 0,
    "sstride mod 2": lambda f: f["ss"] % 2 == 0,
    "k = 256: at least 128 pieces": lambda f: f["pieces"] >= 128 if f["k"] == 256 else None,
}
REC_CLAUSES = {
    "shard base mod 16": lambda f: f["sh"] % 16 == 0,
    "shard base mod 2": lambda f: f["sh"] % 2 == 0,
    "sstride mod 16": lambda f: f["ss"] % 16 == 0,
    "sstride mod 2": lambda f: f["ss"] % 2 == 0,
    "out base mod 8": lambda f: f["out"] % 8 == 0,
    "out base mod 16": lambda f: f["out"] % 16 == 0,
    "ostride mod 8 (batch > 1)": lambda f: f["os"] % 8 == 0 if f["batch"] > 1 else None,
    "ostride mod 16 (batch > 1)": lambda f: f["os"] % 16 == 0 if f["batch"] > 1 else None,
    "batch == 1 with ostride off 8": lambda f: f["batch"] == 1 if f["os"] % 8 else None,
    "present base mod 16": lambda f: f["pr"] % 16 == 0,
    "err_log base mod 16": lambda f: f["el"] % 16 == 0,
    "n = 1024: at least 32 columns": lambda f: f["cols"] >= 32 if (f["n"], f["k"]) == (1024, 256) else None,
    "n = 1024: at least 48 columns": lambda f: f["cols"] >= 48 if (f["n"], f["k"]) == (1024, 256) else None,
}
# (The two 2^32 flattened-space bounds need batches of 2^29 payloads: they are
# checked on the chooser alone, tests/test_dispatch.py.)


@pytest.mark.parametrize("clause", list(ENC_CLAUSES))
def test_encode_clause_has_gpu_cases_on_both_sides(clause):
    sides = {ENC_CLAUSES[clause](f) for f in _enc_facts()} - {None}
    assert sides == {True, False}, clause


@pytest.mark.parametrize("clause", list(REC_CLAUSES))
def test_reconstruct_clause_has_gpu_cases_on_both_sides(clause):
    sides = {REC_CLAUSES[clause](f) for f in _rec_facts()} - {None}
    assert sides == {True, False}, clause


@pytest.mark.parametrize("family,fast", [(256, {"encode_k256w", "encode_kw", "encode_k256_packed"}),
                                         (512, {"encode_k512w"}), (1024, {"encode_k1024"}),
                                         (64, {"encode_kw"})])
def test_each_encode_family_sees_both_sides(family, fast):
    """both sides of every alignment clause within each family of fast
    kernels, not only somewhere in the table"""
    facts = [f for f in _enc_facts() if f["k"] == family and f["pieces"] > 1]
    assert {f["name"] for f in facts} >= fast
    for clause, fn in ENC_CLAUSES.items():
        if clause.startswith("k = 256"):
            continue
        assert {fn(f) for f in facts} - {None} == {True, False}, (family, clause)


@pytest.mark.parametrize("nk,fast", [((1024, 256), {"reconstruct_n1024x", "reconstruct_n1024",
                                                    "reconstruct_n1024_packed"}),
                                     ((2048, 256), {"reconstruct_n4096"}), ((4096, 512), {"reconstruct_n4096"}),
                                     ((4096, 1024), {"reconstruct_n4096"}), ((1024, 128), {"reconstruct_gen"})])
def test_each_reconstruct_family_sees_both_sides(nk, fast):
    facts = [f for f in _rec_facts() if (f["n"], f["k"]) == nk and f["cols"] > 1]
    assert {f["name"] for f in facts} >= fast
    for clause, fn in REC_CLAUSES.items():
        if clause.startswith("n = 1024"):
            continue
        assert {fn(f) for f in facts} - {None} == {True, False}, (nk, clause)


def test_case_ids_are_unique():
    for cases in (L.enc_cases(), L.rec_cases()):
        ids = [L.case_id(c) for c in cases]
        assert len(ids) == len(set(ids))
