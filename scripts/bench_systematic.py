#!/usr/bin/env python3
"""Measurements of the systematic recovery, one JSON line.
Like scripts/bench_ragged.py, the parent commit's library and this tree's are
both loaded into THIS process and take turns on the same resident buffers,
round by round, timed by HIP events on the launch stream.

  bench_systematic.py --parent PATH/liberasure_coding_crust.so [--rounds R] [--steps K] [--big-batch B]

Per shape (4096 x 1 MB at n_validators 1024; 512 x 1 MB at 100, 600, 1500, 3069
and 4096), on the same buffers:
  parent   ECCR_AMD_systematic_batch of the parent library (systematic_g): the baseline
  new      ECCR_AMD_systematic_batch of this tree (the kernel ECCR_AMD_systematic_kernel names)
  copy     a device-to-device copy of k * shard_len * batch bytes: the memory-rate
           yardstick for the same traffic
and whether the two libraries' outputs are equal.  `slower_than_parent` is the
chooser's rule: new's median above parent's median by more than parent's own
round-to-round range.

The config-5 size mix ({15, 300, 5000, 1e5, 1e6, 1e7} B x 16, n_validators
1024): one ECCR_AMD_systematic_ragged call (new) against six uniform calls, one
per size class (parent, and new), and each class's uniform call on its own."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "erasure-coding-crust_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ecc_amd as E  # noqa: E402

MIX = [15, 300, 5000, 10**5, 10**6, 10**7]


def load(path, new):
    L = C.CDLL(path, mode=C.RTLD_LOCAL)
    ul, vp = C.c_ulong, C.c_void_p
    sig = [("ECCR_AMD_systematic_batch", [ul, vp, ul, ul, ul, vp, ul, vp])]
    if new:
        sig += [("ECCR_AMD_systematic_ragged", [ul, vp, vp, ul, ul, vp, vp, vp])]
    L.ECCR_AMD_init_device.restype = E.NPRSResult
    for f, args in sig:
        getattr(L, f).restype = E.NPRSResult
        getattr(L, f).argtypes = args
    assert L.ECCR_AMD_init_device().tag == 0, path
    return L


def P(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def timed(st, fn, steps):
    """mean ms of `steps` back-to-back runs of fn, by events on the stream"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record(st)
    for i in range(steps):
        fn()
        ev[i + 1].record(st)
    torch.cuda.synchronize()
    return statistics.mean(ev[i].elapsed_time(ev[i + 1]) for i in range(steps))


def summary(xs):
    return {"med": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "rounds": [round(x, 4) for x in xs]}


def rounds_of(st, variants, rounds, steps):
    """every variant once per round, the order rotated round by round"""
    t = {v: [] for v in variants}
    names = list(variants)
    for r in range(rounds):
        for v in names[r % len(names):] + names[:r % len(names)]:
            t[v].append(timed(st, variants[v], steps))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the parent commit's liberasure_coding_crust.so")
    ap.add_argument("--big-batch", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--payload", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    old, new = load(a.parent, False), load(E.LIB_PATH, True)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    sp = C.c_void_p(st.cuda_stream)
    ok = lambda r: r.tag == 0 or sys.exit("call failed: " + E.last_error())  # noqa: E731
    res = {"workload": {"payload": a.payload, "rounds": a.rounds, "steps": a.steps}, "shapes": []}
    all_equal = True

    shapes = [(1024, a.big_batch)] + [(nv, a.batch) for nv in (100, 600, 1500, 3069, 4096)]
    for nv, B in shapes:
        n, k, _ = E.code_params(nv)
        sl = E.shard_len(nv, a.payload)
        ss = (sl + 63) // 64 * 64
        d_sh = torch.empty((B, nv, ss), dtype=torch.uint8, device=dev)
        for b0 in range(0, B, 64):  # the k data rows: noise (the reference takes any rows)
            d_sh[b0:b0 + 64, :k] = torch.randint(0, 256, (min(64, B - b0), k, ss), dtype=torch.uint8, device=dev)
        d_out = torch.empty((B, sl * k), dtype=torch.uint8, device=dev)
        d_cpy = torch.empty((B, sl * k), dtype=torch.uint8, device=dev)
        args = (nv, P(d_sh), sl, ss, B, P(d_out), sl * k, sp)
        variants = {"parent": lambda: ok(old.ECCR_AMD_systematic_batch(*args)),
                    "new": lambda: ok(new.ECCR_AMD_systematic_batch(*args)),
                    "copy": lambda: d_cpy.copy_(d_out)}
        outs = {}
        for v in ("parent", "new"):  # warm-up, and the bytes
            d_out.zero_()
            variants[v]()
            torch.cuda.synchronize()
            outs[v] = d_out.clone()
        equal = bool(torch.equal(outs["parent"], outs["new"]))
        # (row 0 of payload 0, column 0 and 1: out symbols 0 and k)
        spot = bool(torch.equal(outs["new"][0, :2], d_sh[0, 0, :2]) and
                    torch.equal(outs["new"][0, 2 * k:2 * k + 2], d_sh[0, 0, 2:4]))
        del outs
        all_equal &= equal and spot
        variants["copy"]()
        t = rounds_of(st, variants, a.rounds, a.steps)
        med = {v: statistics.median(t[v]) for v in t}
        spread = max(t["parent"]) - min(t["parent"])
        moved = 2 * k * sl * B  # bytes read + written
        res["shapes"].append({
            "nv": nv, "k": k, "batch": B, "shard_len": sl,
            "kernel": E.systematic_kernel(nv, d_sh.data_ptr(), sl, ss, B, d_out.data_ptr(), sl * k),
            "equal_to_parent": equal and spot,
            "parent_ms": summary(t["parent"]), "new_ms": summary(t["new"]), "copy_ms": summary(t["copy"]),
            "parent_over_new": round(med["parent"] / med["new"], 3),
            "new_over_copy": round(med["new"] / med["copy"], 3),
            "new_TBps": round(moved / med["new"] / 1e9, 3), "copy_TBps": round(moved / med["copy"] / 1e9, 3),
            "slower_than_parent": bool(med["new"] > med["parent"] + spread)})
        del d_sh, d_out, d_cpy
        torch.cuda.empty_cache()

    # ---------------------------------------------------------------- the config-5 mix
    nv, per = 1024, 16
    n, k, _ = E.code_params(nv)
    lens = [p for p in MIX for _ in range(per)]
    Bm = len(lens)
    items, _, sbytes, obytes = E.ragged_items(nv, lens)
    m_sh = torch.randint(0, 256, (sbytes,), dtype=torch.uint8, device=dev)
    m_out = torch.zeros(obytes, dtype=torch.uint8, device=dev)
    m_items = torch.from_numpy(items.view(np.int64)).to(dev)
    m_st = torch.zeros(2, dtype=torch.int32, device=dev)
    max_s = E.shard_len(nv, max(lens))

    def mix_ragged():
        ok(new.ECCR_AMD_systematic_ragged(nv, P(m_sh), P(m_items), Bm, max_s, P(m_out), P(m_st), sp))

    def one_class(L, c):
        # one uniform batch of a size class: the items of a class are equally spaced in every
        # buffer (ragged_items lays equal lengths out at equal pitches)
        i0 = c * per
        oo, so, sl_, ss_ = (int(items[i0][j]) for j in (0, 2, 3, 4))
        return lambda: ok(L.ECCR_AMD_systematic_batch(nv, P(m_sh, so), sl_, ss_, per, P(m_out, oo),
                                                      int(items[i0 + 1][0]) - oo, sp))

    def mix_classes(L):
        calls = [one_class(L, c) for c in range(len(MIX))]
        return lambda: [f() for f in calls]

    mix = {"parent_six_uniform_calls": mix_classes(old), "new_six_uniform_calls": mix_classes(new),
           "new_one_ragged_call": mix_ragged}
    outs = {}
    for v, fn in mix.items():
        m_out.zero_()
        fn()
        torch.cuda.synchronize()
        outs[v] = m_out.clone()
    mix_equal = all(bool(torch.equal(outs["parent_six_uniform_calls"], o)) for o in outs.values())
    del outs
    tm = rounds_of(st, mix, a.rounds, a.steps)
    res["config5_mix"] = {v: {"ms": summary(tm[v])} for v in mix}
    res["config5_mix"].update({
        "items": Bm, "equal_to_parent": mix_equal, "status_words": m_st.tolist(),
        "kernel": E.systematic_ragged_kernel(nv),
        "ratio_parent_over_ragged": round(statistics.median(tm["parent_six_uniform_calls"]) /
                                          statistics.median(tm["new_one_ragged_call"]), 3)})
    # each size class on its own (16 payloads a call): the small calls, where a launch is most of the time
    res["config5_mix"]["classes"] = []
    for c, p in enumerate(MIX):
        calls = {"parent": one_class(old, c), "new": one_class(new, c)}
        for fn in calls.values():  # calls of ~10 us: settle the launch path before timing them
            timed(st, fn, 100)
        tc = rounds_of(st, calls, a.rounds, 50)
        res["config5_mix"]["classes"].append({
            "payload": p, "parent_ms": summary(tc["parent"]), "new_ms": summary(tc["new"]),
            "slower_than_parent": bool(statistics.median(tc["new"]) > statistics.median(tc["parent"]) +
                                       max(tc["parent"]) - min(tc["parent"]))})
    print(json.dumps(res))
    sys.exit(0 if all_equal and mix_equal else 1)


if __name__ == "__main__":
    main()
