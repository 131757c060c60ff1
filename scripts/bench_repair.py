#!/usr/bin/env python3
"""Measurements of the repair calls, one JSON line: one
process, HIP events on the launch stream, the median and range of `--rounds`
rounds of `--steps` back-to-back calls after a warm-up, the variants of a case
taking turns round by round on the same resident buffers (as
scripts/bench_systematic.py).

  bench_repair.py [--batch 4096] [--payload 1000000] [--rounds 5] [--steps 3]

n_validators 1024.  Case, and what it is compared against (today's way, the
same library, the same buffers):
  repair_random342    repair_batch, 342 random rows present per payload
                      | reconstruct_batch + encode_batch
  repair_10_of_768    repair_batch, 10 rows missing, all in coset 768
                      | reconstruct_batch + encode_batch
  one_parity_row      encode_missing_batch, one wanted parity row per payload
                      | encode_batch
  every_row           encode_missing_batch, every row wanted (what the mask costs)
                      | encode_batch
The locators are computed once per case, outside the timed region, for both
sides.  Every variant leaves the full codeword in the shard buffer, which is
checked against encode_batch's after its warm-up call (`equal`).  `loses`: the
new call's median above its pair's by more than the pair's own round-to-round
range in this run."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "erasure-coding-crust_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ecc_amd as E  # noqa: E402
import synth  # noqa: E402


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
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--payload", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    nv, B, plen = 1024, a.batch, a.payload
    n, k, thr = E.code_params(nv)
    sl = E.shard_len(nv, plen)
    ss, ps, os_ = (sl + 63) // 64 * 64, (plen + 63) // 64 * 64, (sl * k + 63) // 64 * 64
    assert E.lib().ECCR_AMD_init_device().tag == 0, E.last_error()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)

    d_pay = torch.empty((B, ps), dtype=torch.uint8, device=dev)
    for b0 in range(0, B, 256):
        d_pay[b0:b0 + 256] = torch.randint(0, 256, (min(256, B - b0), ps), dtype=torch.uint8, device=dev)
    d_sh = torch.zeros((B, nv, ss), dtype=torch.uint8, device=dev)
    d_out = torch.zeros((B, os_), dtype=torch.uint8, device=dev)
    d_pr = torch.empty((B, n), dtype=torch.uint8, device=dev)
    d_el = torch.zeros((B, n), dtype=torch.int16, device=dev)
    enc_args = (nv, d_pay, plen, ps, B, d_sh, ss)
    E.encode_batch(*enc_args)
    torch.cuda.synchronize()
    full = d_sh.clone()

    def damaged():
        """the shard buffer with every missing row's shard_len bytes overwritten"""
        d_sh.copy_(full)
        gone = torch.nonzero((d_pr[:, :nv] == 0).reshape(-1)).flatten()
        d_sh.view(B * nv, ss)[gone, :sl] = 0x33

    def pair_repair():
        E.reconstruct_batch(nv, d_sh, sl, ss, d_pr, d_el, B, d_out, os_)
        E.encode_batch(nv, d_out, sl * k, os_, B, d_sh, ss)

    def new_repair():
        E.repair_batch(nv, d_sh, sl, ss, d_pr, d_el, B, d_out, os_)

    def new_missing():
        E.encode_missing_batch(*enc_args, d_pr)

    def pair_encode():
        E.encode_batch(*enc_args)

    def present_random(count):
        return synth.present_masks(range(1, B + 1), nv, count, n)

    def present_10_of_768():
        rng = np.random.default_rng(768)
        p = np.zeros((B, n), np.uint8)
        p[:, :nv] = 1
        for b in range(B):
            p[b, 768 + rng.choice(256, 10, replace=False)] = 0
        return p

    def present_one_parity_row():
        rng = np.random.default_rng(1)
        p = np.zeros((B, n), np.uint8)
        p[:, :nv] = 1
        p[np.arange(B), rng.integers(k, nv, B)] = 0
        return p

    cases = [("repair_random342", present_random(thr), new_repair, pair_repair, "reconstruct_batch + encode_batch"),
             ("repair_10_of_768", present_10_of_768(), new_repair, pair_repair, "reconstruct_batch + encode_batch"),
             ("one_parity_row", present_one_parity_row(), new_missing, pair_encode, "encode_batch"),
             ("every_row", np.zeros((B, n), np.uint8), new_missing, pair_encode, "encode_batch")]
    res = {"workload": {"n_validators": nv, "batch": B, "payload": plen, "shard_len": sl, "rounds": a.rounds,
                        "steps": a.steps, "encode_missing_kernel": E.encode_missing_kernel(*enc_args),
                        "encode_kernel": E.encode_kernel(*enc_args),
                        "repair_encode_stage_kernel": E.encode_missing_kernel(nv, d_out, sl * k, os_, B, d_sh, ss)},
           "cases": []}
    all_equal = True
    for name, pres, new, pair, pair_name in cases:
        d_pr.copy_(torch.from_numpy(np.ascontiguousarray(pres)))
        E.error_locator(nv, d_pr, B, d_el)
        equal = {}
        for v, fn in (("new", new), ("pair", pair)):  # warm-up, and the bytes
            damaged()
            assert not torch.equal(d_sh, full)  # (the check below can fail)
            fn()
            torch.cuda.synchronize()
            equal[v] = bool(torch.equal(d_sh, full))
        all_equal &= equal["new"] and equal["pair"]
        t = rounds_of(st, {"new": new, "pair": pair}, a.rounds, a.steps)
        med = {v: statistics.median(t[v]) for v in t}
        spread = max(t["pair"]) - min(t["pair"])
        res["cases"].append({"case": name, "compared_against": pair_name,
                             "rows_missing_per_payload": round(float((pres[:, :nv] == 0).sum()) / B, 2),
                             "new_ms": summary(t["new"]), "pair_ms": summary(t["pair"]),
                             "pair_over_new": round(med["pair"] / med["new"], 3), "equal": equal,
                             "loses": bool(med["new"] > med["pair"] + spread)})
    print(json.dumps(res))
    sys.exit(0 if all_equal else 1)


if __name__ == "__main__":
    main()
