#!/usr/bin/env python3
"""Generate tests/golden/locator_zero.json: erasure patterns whose locator is
== 0 (mod 65535) at a row the reconstruct actually uses.

A locator entry is a log mod 65535, so 0 and 65535 both mean "multiply by one";
in the kernels the raw value 65535 is also the index of the multiply-by-zero
table and the "row absent" mark of the gather order.  About one used entry in
65535 is == 0, so random patterns meet the case by luck only.  This script
searches seeded random present sets with the project's own oracle restatement
(oracle.Oracle().error_poly; nothing is read from the reference tree) until it
has, for every n_validators of NVS,

  pattern P: some present row v < n_validators has E[v] == 0 (mod 65535)
             (decode_main scales the received symbol by E[v]) and some row
             below k is erased (with every row below k present the output is
             a copy of the received rows and no scaled symbol reaches it),
  pattern S: some erased row y < k has E[y] == 0 (mod 65535)
             (decode_main scales the recovered symbol by E[y]).

The file stores the masks themselves (bit v of the hex string's byte v / 8, low
bit first, n bits), not seeds, so it does not depend on numpy's generator; the
rows listed under "zero" are every used row (present rows below n_validators,
erased rows below k) whose log is == 0.  tests/test_locator_contract.py
recomputes all of it.

    python tests/golden/make_locator_zero.py
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle as orc  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "locator_zero.json")
NVS = [2, 3, 6, 20, 46, 100, 300, 600, 765, 766, 800, 1024, 1500, 2048, 2500, 3070, 4096, 5000,
       16384, 65536]
KINDS = ("P", "S")
CAP = 60_000  # tries per n_validators


def mask_to_hex(mask: np.ndarray) -> str:
    return np.packbits(np.asarray(mask, np.uint8) != 0, bitorder="little").tobytes().hex()


def mask_from_hex(text: str, n: int) -> np.ndarray:
    """present flags [n] (0 / 1) of a stored mask"""
    bits = np.unpackbits(np.frombuffer(bytes.fromhex(text), np.uint8), bitorder="little")
    assert bits.size == max(n, 8) // 8 * 8 and not bits[n:].any(), "mask length"
    return bits[:n].copy()


def locator(o, mask: np.ndarray, nv: int, n: int) -> np.ndarray:
    """the oracle's locator row [n] (raw uint16) of a present mask"""
    erased = (np.asarray(mask[:n]) == 0).astype(np.uint8)
    erased[nv:] = 1
    return o.error_poly(erased, n)[:n].copy()


def zero_rows(mask: np.ndarray, el: np.ndarray, nv: int, k: int):
    """(present rows < nv, erased rows < k) whose log is == 0 (mod 65535)"""
    z = el.astype(np.int64) % 65535 == 0
    pres = np.asarray(mask) != 0
    v = np.arange(len(mask))
    return (np.flatnonzero(z & pres & (v < nv)).tolist(), np.flatnonzero(z & ~pres & (v < k)).tolist())


def search(o, nv: int):
    n, k = o.params(nv)
    thr = o.threshold(nv)
    rng = np.random.default_rng(0x10CA7 + nv)
    found = {}
    for t in range(CAP):
        size = thr if t % 2 == 0 else int(rng.integers(k, nv + 1))
        mask = np.zeros(n, np.uint8)
        mask[rng.permutation(nv)[:size]] = 1
        zp, zs = zero_rows(mask, locator(o, mask, nv, n), nv, k)
        for kind, hit in (("P", zp and not mask[:k].all()), ("S", zs)):
            if hit and kind not in found:
                found[kind] = dict(present=mask_to_hex(mask), zero=sorted(zp + zs), tries=t + 1)
        if len(found) == len(KINDS):
            return n, k, found
    raise SystemExit(f"n_validators {nv}: no pattern of kind(s) "
                     f"{[x for x in KINDS if x not in found]} in {CAP} tries")


def main():
    # the restatement alone: no need for the HIP library or the reference build
    subprocess.run(["make", "-s", "-C", orc.HERE, orc.ORACLE_SO], check=True)
    o = orc.Oracle()
    cases = {}
    for nv in NVS:
        n, k, found = search(o, nv)
        cases[str(nv)] = dict(n=n, k=k, **{kind: found[kind] for kind in KINDS})
        print(f"nv {nv}: n {n} k {k} " + " ".join(f"{x}: try {found[x]['tries']} rows {found[x]['zero']}"
                                                for x in KINDS), flush=True)
    with open(OUT, "w") as f:
        json.dump(dict(comment="tests/golden/make_locator_zero.py: present masks (hex, bit v of byte "
                               "v / 8, low bit first) whose locator is 0 mod 65535 at the used rows "
                               "'zero'", cases=cases), f, indent=1)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
