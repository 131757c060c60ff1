#!/usr/bin/env python3
"""Measurements of the ragged device-batch calls, one JSON
line.  Like scripts/ab_inproc.py, the parent commit's library and this tree's
are both loaded into THIS process and take turns on the same resident
buffers, round by round, timed by HIP events on the launch stream.

  bench_ragged.py --parent PATH/liberasure_coding_crust.so [--diag PATH/diag.so] [--batch B] [--rounds R] [--steps K]

1. uniform:  ECCR_AMD_encode_batch / reconstruct_batch, parent against new
             (B x 1 MB, n_validators 1024, threshold present): the
             no-regression check of the shared kernel bodies.
2. equal:    a ragged batch of B equal 1 MB items (new library) against the
             parent's uniform calls on the same buffers; `plan_ms` = the plan
             kernel alone (a ragged encode of one 15-byte item costs little else).
3. mix:      the config-5 mix {15, 300, 5000, 1e5, 1e6, 1e7} B x 16 each,
             device-resident, one random threshold pattern per item: one
             ragged encode + locator + one ragged reconstruct (new) against six
             uniform encodes + locators + reconstructs, one per size class (parent)."""
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
import synth  # noqa: E402

NV = 1024
MIX = [15, 300, 5000, 10**5, 10**6, 10**7]


def load(path, ragged):
    L = C.CDLL(path, mode=C.RTLD_LOCAL)
    ul, vp = C.c_ulong, C.c_void_p
    sig = [("ECCR_AMD_encode_batch", [ul, vp, ul, ul, ul, vp, ul, vp]),
           ("ECCR_AMD_error_locator", [ul, vp, ul, vp, vp]),
           ("ECCR_AMD_reconstruct_batch", [ul, vp, ul, ul, vp, vp, ul, vp, ul, vp])]
    if ragged:
        sig += [("ECCR_AMD_encode_ragged", [ul, vp, vp, ul, ul, vp, vp, vp]),
                ("ECCR_AMD_reconstruct_ragged", [ul, vp, vp, vp, vp, vp, ul, ul, vp, vp, vp])]
    L.ECCR_AMD_init_device.restype = E.NPRSResult
    for f, args in sig:
        getattr(L, f).restype = E.NPRSResult
        getattr(L, f).argtypes = args
    assert L.ECCR_AMD_init_device().tag == 0, path
    return L


def P(t):
    return C.c_void_p(t.data_ptr())


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the parent commit's liberasure_coding_crust.so")
    ap.add_argument("--diag", help="a diagnostic build (scripts/variants/ragged_div.py: the lookup replaced by "
                    "the division) timed beside the others on the equal-items batch")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--payload", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    old, new = load(a.parent, False), load(E.LIB_PATH, True)
    diag = load(a.diag, True) if a.diag else None
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    sp = C.c_void_p(st.cuda_stream)
    n, k, thr = E.code_params(NV)
    ok = lambda r: r.tag == 0 or sys.exit("call failed: " + E.last_error())  # noqa: E731
    res = {"workload": {"nv": NV, "batch": a.batch, "payload": a.payload, "rounds": a.rounds, "steps": a.steps}}

    # ---------------------------------------------------------------- 1 + 2
    B, plen = a.batch, a.payload
    sl = E.shard_len(NV, plen)
    ss = (sl + 63) // 64 * 64
    d_pay = torch.empty((B, plen), dtype=torch.uint8, device=dev)
    for c0 in range(0, B, 256):
        d_pay[c0:c0 + 256] = synth.payloads_torch(list(range(c0, min(B, c0 + 256))), plen, device=dev)
    d_pres = torch.from_numpy(synth.present_masks([10**6 + s for s in range(B)], NV, thr, n)).to(dev)
    d_sh = torch.empty((B, NV, ss), dtype=torch.uint8, device=dev)
    d_el = torch.empty((B, n), dtype=torch.int16, device=dev)
    d_out = torch.empty((B, sl * k), dtype=torch.uint8, device=dev)
    d_st = torch.zeros(4, dtype=torch.int32, device=dev)
    assert plen % 16 == 0, "equal-items layout: a payload pitch that is a multiple of 16"
    enc_items = np.array([(b * plen, plen, b * NV * ss, sl, ss) for b in range(B)], np.uint64)
    rec_items = enc_items.copy()
    rec_items[:, 0] = [b * sl * k for b in range(B)]
    d_ie = torch.from_numpy(enc_items.view(np.int64)).to(dev)
    d_ir = torch.from_numpy(rec_items.view(np.int64)).to(dev)
    tiny = torch.from_numpy(np.array([(0, 15, 0, 2, 16)], np.uint64).view(np.int64)).to(dev)

    def uni(L):
        return (lambda: ok(L.ECCR_AMD_encode_batch(NV, P(d_pay), plen, plen, B, P(d_sh), ss, sp)),
                lambda: ok(L.ECCR_AMD_reconstruct_batch(NV, P(d_sh), sl, ss, P(d_pres), P(d_el), B, P(d_out),
                                                        sl * k, sp)))

    def rag(L):
        return (lambda: ok(L.ECCR_AMD_encode_ragged(NV, P(d_pay), P(d_ie), B, plen, P(d_sh), P(d_st), sp)),
                lambda: ok(L.ECCR_AMD_reconstruct_ragged(NV, P(d_sh), P(d_ir), P(d_pres), P(d_el), None, B, sl,
                                                         P(d_out), P(d_st[2:]), sp)))

    variants = {"parent_uniform": uni(old), "new_uniform": uni(new), "new_ragged": rag(new)}
    if diag:
        variants["diag_ragged_division"] = rag(diag)
    ok(new.ECCR_AMD_error_locator(NV, P(d_pres), B, P(d_el), sp))
    t = {v: {"encode": [], "reconstruct": []} for v in variants}
    good = {}
    for v, (enc, rec) in variants.items():  # warm-up and round trip
        d_sh.zero_()
        d_out.zero_()
        enc()
        rec()
        torch.cuda.synchronize()
        good[v] = bool(torch.equal(d_out[:, :plen], d_pay))
    names = list(variants)
    for r in range(a.rounds):
        for v in names[r % len(names):] + names[:r % len(names)]:
            enc, rec = variants[v]
            t[v]["encode"].append(timed(st, enc, a.steps))
            t[v]["reconstruct"].append(timed(st, rec, a.steps))
    res["uniform_and_equal"] = {v: {"ok": good[v], "encode_ms": summary(t[v]["encode"]),
                                    "reconstruct_ms": summary(t[v]["reconstruct"])} for v in variants}
    tiny_sh = torch.empty(NV * 16, dtype=torch.uint8, device=dev)
    plan = lambda: ok(new.ECCR_AMD_encode_ragged(NV, P(d_pay), P(tiny), 1, 15, P(tiny_sh), None, sp))  # noqa: E731
    plan()
    res["uniform_and_equal"]["plan_ms"] = {"one_15B_item_call": round(timed(st, plan, 50), 4)}
    stat = d_st.tolist()
    del d_pay, d_sh, d_out, d_el, d_pres, d_ie, d_ir
    torch.cuda.empty_cache()

    # ---------------------------------------------------------------- 3: the config-5 mix
    per = 16
    lens = [p for p in MIX for _ in range(per)]
    Bm = len(lens)
    items, pbytes, sbytes, obytes = E.ragged_items(NV, lens)
    m_pay = torch.zeros(pbytes, dtype=torch.uint8, device=dev)
    for i, (it, p) in enumerate(zip(items, lens)):
        m_pay[int(it[0]): int(it[0]) + p] = synth.payloads_torch([1000 + i], p, device=dev)[0]
    m_sh = torch.zeros(sbytes, dtype=torch.uint8, device=dev)
    m_out = torch.zeros(obytes, dtype=torch.uint8, device=dev)
    m_pres = torch.from_numpy(synth.present_masks([2 * 10**6 + s for s in range(Bm)], NV, thr, n)).to(dev)
    m_el = torch.empty((Bm, n), dtype=torch.int16, device=dev)
    m_items = torch.from_numpy(items.view(np.int64)).to(dev)
    max_p, max_s = max(lens), E.shard_len(NV, max(lens))

    def mix_ragged():
        ok(new.ECCR_AMD_encode_ragged(NV, P(m_pay), P(m_items), Bm, max_p, P(m_sh), None, sp))
        ok(new.ECCR_AMD_error_locator(NV, P(m_pres), Bm, P(m_el), sp))
        ok(new.ECCR_AMD_reconstruct_ragged(NV, P(m_sh), P(m_items), P(m_pres), P(m_el), None, Bm, max_s, P(m_out),
                                           None, sp))

    def mix_classes(L):
        # one uniform batch per size class: the items of a class are equally spaced in every
        # buffer (ragged_items lays equal lengths out at equal pitches)
        def run():
            for c, p in enumerate(MIX):
                i0 = c * per
                po, so, ss_ = int(items[i0][0]), int(items[i0][2]), int(items[i0][4])
                pitch = int(items[i0 + 1][0]) - po
                sl_ = E.shard_len(NV, p)
                ok(L.ECCR_AMD_encode_batch(NV, C.c_void_p(m_pay.data_ptr() + po), p, pitch, per,
                                           C.c_void_p(m_sh.data_ptr() + so), ss_, sp))
                ok(L.ECCR_AMD_error_locator(NV, C.c_void_p(m_pres.data_ptr() + i0 * n), per,
                                            C.c_void_p(m_el.data_ptr() + i0 * n * 2), sp))
                ok(L.ECCR_AMD_reconstruct_batch(NV, C.c_void_p(m_sh.data_ptr() + so), sl_, ss_,
                                                C.c_void_p(m_pres.data_ptr() + i0 * n),
                                                C.c_void_p(m_el.data_ptr() + i0 * n * 2), per,
                                                C.c_void_p(m_out.data_ptr() + po), pitch, sp))
        return run

    mix = {"parent_six_uniform_calls": mix_classes(old), "new_six_uniform_calls": mix_classes(new),
           "new_one_ragged_call": mix_ragged}
    tm, goodm = {v: [] for v in mix}, {}
    for v, fn in mix.items():
        m_sh.zero_()
        m_out.zero_()
        fn()
        torch.cuda.synchronize()
        goodm[v] = all(bool(torch.equal(m_out[int(it[0]): int(it[0]) + p], m_pay[int(it[0]): int(it[0]) + p]))
                       for it, p in zip(items, lens))
    names = list(mix)
    for r in range(a.rounds):
        for v in names[r % 3:] + names[:r % 3]:
            tm[v].append(timed(st, mix[v], a.steps))
    res["config5_mix"] = {v: {"ok": goodm[v], "ms": summary(tm[v])} for v in mix}
    res["config5_mix"]["items"] = Bm
    res["config5_mix"]["ratio_parent_over_ragged"] = round(
        statistics.median(tm["parent_six_uniform_calls"]) / statistics.median(tm["new_one_ragged_call"]), 3)
    res["status_words"] = stat
    print(json.dumps(res))
    bad = [v for v, g in {**good, **goodm}.items() if not g]
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
