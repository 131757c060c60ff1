"""The shapes at which every persistent kernel runs past its first tile per
workgroup (test_tile_loops.py runs every one of them).

Every fast kernel sizes its grid as min(tiles, c x CUs) and loops over tiles:
from a ticket counter, a static grid stride, a contiguous range or XCD spans.
The code that only runs when a workgroup (or, in the packed forms, a wave)
takes a second tile - the next tile's prefetch, the reload of per-payload
tables, the reload of table image 0, the barrier for the previous tile's
readers, the switch of the packed mapping - needs more tiles than the grid
has workgroups, so the shapes here are functions of the CU count.

The tile geometry and the grid rule of each kernel are recorded here as
LITERALS (ENC_QUEUE, REC_GEN_TILE, ...), not read from the sources: the
kernel-name queries and the CPU tests of test_tile_loops.py keep them honest.
`plan(C)` returns the cases for a device of C compute units; each case carries
the conditions (`why`: text -> bool) it is there to meet, which the tests
assert before anything is launched, and the static schedule (`units`, `sched`)
from which `static_counts` computes how many workgroups (waves) run a second
and a third tile.  None of that enumeration ever yields an expected byte."""
from collections import namedtuple

import ecc_amd as E
import nv_boundaries as NB

WAVES = 8  # waves per workgroup of every kernel here but encode_k256_packed (16)

# ------------------------------------------------------------------ the plan table
# encodes with a tile queue: (n, k) -> (kernel, pieces per tile, workgroups per CU).
# A piece is 2 k payload bytes = one shard column; encode_kw's tile is 32 KB of
# payload (16384 / k pieces).  Schedule: ticket counter, static grid stride with a
# NULL workspace.
ENC_QUEUE = {
    (64, 16): ("encode_kw", 1024, 2), (128, 16): ("encode_kw", 1024, 2),
    (128, 32): ("encode_kw", 512, 2), (256, 32): ("encode_kw", 512, 2),
    (256, 64): ("encode_kw", 256, 2), (512, 64): ("encode_kw", 256, 2),
    (512, 128): ("encode_kw", 128, 2), (1024, 128): ("encode_kw", 128, 2),
    (2048, 256): ("encode_kw", 64, 2),  # from 128 pieces; below: encode_k256_packed
    (2048, 512): ("encode_k512w", 32, 2), (4096, 512): ("encode_k512w", 32, 2),
    (1024, 256): ("encode_k256w", 64, 2),  # from 128 pieces; below: encode_k256_packed
    (4096, 1024): ("encode_k1024", 32, 1),
}
K256_MIN_PIECES = 128  # k = 256: payloads below run encode_k256_packed
# encode_k256_packed, n = 1024: 16 waves per workgroup, grid = min(tasks, CUs), a
# wave task = 8 pieces of the exactly flattened piece space, static wave stride
PACKED_ENC_WAVES, PACKED_TASK = 16, 8
# encode_k256_packed, n = 2048: tiles of 128 slots, a payload's pieces rounded up
# to 8 slots, grid = min(tiles, CUs), static stride; every tile ends on table image 1
PACKED_TILE, PACKED_ROUND = 128, 8
# reconstruct_gen: n -> shard columns per tile (32768 / n); grid = min(tiles, CUs),
# workgroup w runs the contiguous range [per w, per (w + 1)), per = ceil(T / grid)
REC_GEN_TILE = {64: 512, 128: 256, 256: 128, 512: 64, 1024: 32}
REC_GEN = ((64, 16), (128, 16), (128, 32), (256, 32), (256, 64), (512, 64), (512, 128), (1024, 128))
# reconstruct_n4096: 32 columns per tile (4 per wave), grid = min(tiles, CUs); n =
# 2048 static, n = 4096 a TileQueue; one stride / counter below 8 x grid tiles, 8
# contiguous spans from there (grids that are a multiple of 8)
REC_N4096 = ((2048, 256), (2048, 512), (4096, 512), (4096, 1024))
N4096_COLS, SPANS = 32, 8
# reconstruct_n1024 (32 .. 47 columns): 32 columns per tile, grid = min(tiles, CUs),
# static stride, metadata loaded one tile ahead
N1024_COLS = 32
# reconstruct_n1024_packed: a wave step = one group of 4 columns of the flattened
# space (columns rounded up to 4 per payload), grid = min(groups, CUs) x 8 waves;
# group g on (workgroup g % grid, wave g / grid) ("spread") below 2 x grid x 8
# groups, on (workgroup g / 8 % grid, wave g % 8) ("adjacent") from there
N1024_GROUP = 4
GRID_Y = 65535  # the generic kernels: payload slots in gridDim.y, b += gridDim.y past it

D = 5  # basis payloads; payload b = the XOR of those selected by the bits of b % 31 + 1
COMBOS = (1 << D) - 1
PATTERNS = ("P0", "P1", "P2", "K")  # pattern of payload b: PATTERNS[b % 4] (period coprime to 3 tiles)

Case = namedtuple("Case", "op kernel tag nv plen batch off ps ss os form T units sched tile why")
# op      "encode" | "reconstruct" | "generic"
# kernel  the literal the kernel-name query must return (generic: encode, reconstruct, systematic)
# off, ps, ss, os  payload base offset and pitch, shard pitch, out pitch (bytes)
# form    encode: "ticket" | "static" (encode_batch_ws with a NULL workspace) | "plain"
# T, units, sched  tiles (tasks, groups), scheduled units (workgroups or waves) and how they
#         walk: "stride" | "range" | "spans" | "adjacent" | "grid_y"
# tile    (slots per payload, slots per tile) of the flattened column space, to name the tile
#         of a wrong byte


def up(x, a):
    return (x + a - 1) // a * a


def nv_of(n, k):
    """hi - 1 of the class: a partly filled last coset and the most cosets"""
    (c,) = [c for c in NB.classes() if (c.n, c.k) == (n, k)]
    assert c.hi - 1 > c.lo and (c.hi - 1) % k != 0
    return c.hi - 1


def guard_pitches(nv, plen):
    """(payload pitch, shard pitch, out pitch): 64-B multiples; the shard and out
    pitches 64 bytes past the rounded length, so every row and output has a gap"""
    _, k, _ = E.code_params(nv)
    sl = E.shard_len(nv, plen)
    return up(plen, 64), up(sl, 64) + 64, up(sl * k, 64) + 64


def pieces_len(k, pieces):
    """`pieces` pieces (= shard columns) with a ragged byte tail"""
    return 2 * k * pieces - 3


def next_batch(b, ok):
    while not ok(b):
        b += 1
    return b


def _case(op, kernel, tag, nv, plen, batch, form, T, units, sched, tile, why, off=0, pitches=None):
    ps, ss, os_ = pitches or guard_pitches(nv, plen)
    return Case(op, kernel, tag, nv, plen, batch, off, ps, ss, os_, form, T, units, sched, tile, why)


# ------------------------------------------------------------------ encodes with a tile queue
def encode_queue_cases(C):
    out = []
    for i, ((n, k), (kernel, tile, per_cu)) in enumerate(sorted(ENC_QUEUE.items())):
        nv, S, wp = nv_of(n, k), per_cu * C, tile // WAVES
        # "several tiles each": two whole tiles and a partial one, some of whose waves have no piece
        part = tile // 2 + 1
        pieces = 2 * tile + part
        plen = pieces_len(k, pieces)
        batch = next_batch(5 * S // 6 + 1, lambda b: (3 * b) % S != 0)
        T = 3 * batch
        why = {
            "three tiles per payload": E.shard_len(nv, plen) == 2 * pieces and -(-pieces // tile) == 3,
            "the last tile has populated and empty waves": 1 <= -(-part // wp) < WAVES and part % wp != 0,
            "a ragged byte tail": plen % (2 * k) != 0,
            "every workgroup of the static form runs two tiles": 2 * S < T,
            "some run three": T % S != 0,
            "k = 256 stays above the packed form": k != 256 or pieces >= K256_MIN_PIECES,
        }
        for form in ("ticket", "static"):
            out.append(_case("encode", kernel, "several-%d-%d" % (n, k), nv, plen, batch, form, T, S, "stride",
                             (3 * tile, tile), why))
        if k == 256:  # below 128 pieces k = 256 runs the packed form: packed_encode_cases
            continue
        # "many one-tile payloads": every tile of a workgroup another payload, most waves empty
        pieces = 1 if i % 2 == 0 else wp + 1
        plen = pieces_len(k, pieces)
        batch = 2 * S + S // 2 + 3
        why = {
            "one tile per payload": E.shard_len(nv, plen) == 2 * pieces and pieces <= tile,
            "one or two populated waves": -(-pieces // wp) == (1 if pieces == 1 else 2),
            "every workgroup runs two tiles": batch > 2 * S,
            "some run three": batch % S != 0,
        }
        for form in ("ticket", "static"):
            out.append(_case("encode", kernel, "many-%d-%d" % (n, k), nv, plen, batch, form, batch, S, "stride",
                             (tile, tile), why))
    return out


# ------------------------------------------------------------------ packed encodes
def packed_layout(nv, plen, layout):
    """(payload base offset, payload pitch, shard pitch, out pitch) of
    test_packed_small_batches' "tight" and "odd" layouts"""
    _, k, _ = E.code_params(nv)
    sl = E.shard_len(nv, plen)
    assert layout in ("tight", "odd")
    return (0, plen, sl, sl * k) if layout == "tight" else (1, plen + 3, sl + 2, sl * k)


def packed_encode_cases(C):
    out = []
    for nv in (1023, 766):  # n = 1024: wave tasks of 8 pieces over CUs x 16 waves
        for plen, pieces in ((15, 1), (1100, 3)):
            units = C * PACKED_ENC_WAVES
            tasks = 2 * units + units // 2 + 3
            batch = next_batch(-(-PACKED_TASK * (tasks - 1) // pieces) + 1,
                               lambda b: (b * pieces) % PACKED_TASK != 0 and -(-b * pieces // PACKED_TASK) >= tasks)
            T = -(-batch * pieces // PACKED_TASK)
            why = {
                "pieces per payload": E.shard_len(nv, plen) == 2 * pieces and pieces < K256_MIN_PIECES,
                "every wave runs two tasks": T > 2 * units,
                "some run three": T % units != 0,
                "the last task is partial": (batch * pieces) % PACKED_TASK != 0,
                "a task's 8 pieces straddle payloads": PACKED_TASK % pieces != 0 or pieces == 1,
            }
            for layout in ("tight", "odd"):
                off, ps, ss, os_ = packed_layout(nv, plen, layout)
                out.append(_case("encode", "encode_k256_packed", "%dB-%s" % (plen, layout), nv, plen, batch, "plain",
                                 T, units, "stride", (pieces, PACKED_TASK), why, off, (ps, ss, os_)))
    for nv in (1532, 1025):  # n = 2048: 128-slot tiles over CUs workgroups, the image reload
        for plen, pieces in ((300, 1), (5000, 10)):
            npp8 = up(pieces, PACKED_ROUND)
            tiles = 2 * C + C // 2 + 3
            batch = next_batch(-(-PACKED_TILE * (tiles - 1) // npp8) + 1,
                               lambda b: -(-b * npp8 // PACKED_TILE) % C != 0 and -(-b * npp8 // PACKED_TILE) >= tiles)
            T = -(-batch * npp8 // PACKED_TILE)
            why = {
                "slots per payload": E.shard_len(nv, plen) == 2 * pieces and npp8 == (8 if pieces == 1 else 16),
                "every workgroup reloads image 0 (a second tile)": T > 2 * C,
                "some run three": T % C != 0,
                "every tile ends on image 1": nv > 1024,
                "dead slots in every payload": npp8 - pieces == (7 if pieces == 1 else 6),
            }
            for layout in ("tight", "odd"):
                off, ps, ss, os_ = packed_layout(nv, plen, layout)
                out.append(_case("encode", "encode_k256_packed", "%dB-%s" % (plen, layout), nv, plen, batch, "plain",
                                 T, C, "stride", (npp8, PACKED_TILE), why, off, (ps, ss, os_)))
    return out


# ------------------------------------------------------------------ reconstructs
def range_transitions(T, grid, tiles_pp=3):
    """reconstruct_gen's contiguous ranges: which steps tile -> tile + 1 happen
    inside some workgroup's range, for payloads of two whole tiles and a partial
    one.  Serves the plan only."""
    per = -(-T // grid)
    seen = set()
    for w in range(grid):
        for t in range(per * w, min(per * (w + 1), T) - 1):
            seen.add(("whole->whole, the prefetch consumed", "whole->partial, nothing prefetched",
                      "payload->next payload, the tables reloaded")[t % tiles_pp])
    return per, seen


def reconstruct_gen_cases(C):
    out = []
    for n, k in REC_GEN:
        nv, tc = nv_of(n, k), REC_GEN_TILE[n]
        part = tc // 2 + 1
        cols = 2 * tc + part
        plen = pieces_len(k, cols)
        batch = 5 * C // 3
        T = 3 * batch
        grid = min(T, C)
        per, seen = range_transitions(T, grid)
        why = {
            "three tiles per payload": E.shard_len(nv, plen) == 2 * cols and -(-cols // tc) == 3,
            "the last tile has idle waves": 1 <= -(-part // (tc // WAVES)) < WAVES,
            "ranges of four tiles or more": per >= 4,
            "ranges out of step with the payloads": per % 3 != 0,
            "all three transitions inside a range": len(seen) == 3,
        }
        out.append(_case("reconstruct", "reconstruct_gen", "%d-%d" % (n, k), nv, plen, batch, None, T, grid, "range",
                         (3 * tc, tc), why))
    return out


def span_ranges(T, grid):
    """xcd_span's 8 contiguous spans [(first tile, end)], or None below 8 x grid tiles"""
    if grid % SPANS != 0 or T < SPANS * grid:
        return None
    chunk = -(-T // SPANS)
    return [(x * chunk, min(x * chunk + chunk, T)) for x in range(SPANS)]


def reconstruct_n4096_cases(C):
    out = []
    cols = 2 * N4096_COLS + 6  # 70 columns: the last tile has 6, waves 2 .. 7 idle
    for n, k in REC_N4096:
        nv = nv_of(n, k)
        plen = pieces_len(k, cols)
        batch = next_batch(5 * C // 6 + 1, lambda b: (3 * b) % C != 0)
        T = 3 * batch
        why = {
            "three tiles per payload, the last of 6 columns": E.shard_len(nv, plen) == 2 * cols,
            "a single range / counter": C < T < SPANS * C and span_ranges(T, min(T, C)) is None,
            "some workgroups run one tile more": T % C != 0,
        }
        out.append(_case("reconstruct", "reconstruct_n4096", "single-%d-%d" % (n, k), nv, plen, batch, None, T, C,
                         "stride", (3 * N4096_COLS, N4096_COLS), why))
        if n != 2048:  # the span regime of n = 4096: test_gpu_parity.test_batch_xcd_spans
            continue

        def inside(b):
            sp = span_ranges(3 * b, C)
            return sp is not None and (3 * b) % SPANS != 0 and any(lo % 3 for lo, _ in sp) and any(hi % 3 for _, hi in sp)

        batch = next_batch(-(-SPANS * C // 3), inside)
        T = 3 * batch
        sp = span_ranges(T, C)
        why = {
            "three tiles per payload, the last of 6 columns": E.shard_len(nv, plen) == 2 * cols,
            "eight spans (a grid of a multiple of 8 workgroups)": sp is not None and T >= SPANS * C,
            "uneven spans": T % SPANS != 0,
            "spans begin and end inside a payload": sp is not None and any(lo % 3 for lo, _ in sp) and any(
                hi % 3 for _, hi in sp),
        }
        out.append(_case("reconstruct", "reconstruct_n4096", "spans-%d-%d" % (n, k), nv, plen, batch, None, T, C,
                         "spans", (3 * N4096_COLS, N4096_COLS), why))
    return out


def reconstruct_n1024_cases(C):
    """With an even grid a workgroup keeps the parity of its tile index, so in the
    40-column shape (whole tile, 8-column tile, ...) a workgroup runs whole tiles
    only or partial tiles only: whole -> partial inside one workgroup cannot occur
    here (it does in reconstruct_gen and reconstruct_n4096)."""
    out = []
    for nv in (1023, 766):
        for cols, batch in ((32, 2 * C + C // 2 + 3), (40, C + C // 4 + 3)):
            plen = pieces_len(256, cols)
            tpp = -(-cols // N1024_COLS)
            T = tpp * batch
            why = {
                "columns": E.shard_len(nv, plen) == 2 * cols and 32 <= cols < 48,
                "more payloads than workgroups": batch > (2 * C if cols == 32 else C),
                "every workgroup runs two tiles": T > 2 * C,
                "some run one more": T % C != 0,
            }
            out.append(_case("reconstruct", "reconstruct_n1024", "%dcols" % cols, nv, plen, batch, None, T, C,
                             "stride", (tpp * N1024_COLS, N1024_COLS), why))
    return out


def reconstruct_n1024_packed_cases(C):
    out = []
    W = C * WAVES
    for nv in (1023, 800):
        for tag, cols, batch in (("spread", 1, W + W // 2 + 5), ("adjacent", 1, 2 * W + W // 4 + 101),
                                 ("adjacent3", 10, next_batch(2 * W // 3 + W // 8 + 1, lambda b: b % 8 != 0))):
            plen = pieces_len(256, cols)
            sl = E.shard_len(nv, plen)
            gpp = up(cols, N1024_GROUP) // N1024_GROUP
            T = gpp * batch
            spread = T < 2 * W
            why = {
                "columns": sl == 2 * cols and cols < 32,
                "the mapping": spread == (tag == "spread"),
                "a second wave step": T > W,
                "the last step is partial": T % W != 0,
            }
            if tag == "spread":
                why["below the switch"] = W < T < 2 * W
            elif tag == "adjacent":
                why["past the switch"] = T >= 2 * W + 100
            else:
                why["a workgroup's 8 adjacent groups straddle payloads"] = gpp == 3 and batch % 8 != 0 and T >= 2 * W
            for ptag, extra in (("tight", 0), ("pitch+2", 2)):
                out.append(_case("reconstruct", "reconstruct_n1024_packed", "%s-%s" % (tag, ptag), nv, plen, batch,
                                 None, T, W, "stride" if spread else "adjacent", (gpp * N1024_GROUP, N1024_GROUP), why,
                                 0, (up(plen, 64), sl + extra, up(sl * 256, 64) + 64)))
    return out


def generic_cases(C):
    """encode_g, reconstruct_g and systematic_g past gridDim.y (LDS forms: no scratch)"""
    out = []
    for nv in (6, 20):
        batch = GRID_Y + 37
        n, k, _ = E.code_params(nv)
        why = {"a second pass of b += gridDim.y": GRID_Y < batch < 2 * GRID_Y, "the LDS forms": n <= 4096 and k < 16,
               "one column": E.shard_len(nv, 3) == 2}
        out.append(_case("generic", ("encode_g", "reconstruct_g", "systematic_g"), "batch%d" % batch, nv, 3, batch,
                         "plain", batch, GRID_Y, "grid_y", (1, 1), why))
    return out


def plan(C):
    """every case for a device of C compute units"""
    return (encode_queue_cases(C) + packed_encode_cases(C) + reconstruct_gen_cases(C) + reconstruct_n4096_cases(C) +
            reconstruct_n1024_cases(C) + reconstruct_n1024_packed_cases(C) + generic_cases(C))


def case_id(c):
    name = c.kernel if isinstance(c.kernel, str) else "generic"
    return "%s-nv%d-%s%s" % (name, c.nv, c.tag, "-" + c.form if c.form in ("ticket", "static") else "")


# ------------------------------------------------------------------ what a case costs and covers
def allocations(c):
    """bytes of the device buffers a case holds at once: payloads, shards, flags,
    locators, outputs"""
    n, _, _ = E.code_params(c.nv)
    a = {"payloads": c.off + c.batch * c.ps + 8, "shards": c.batch * c.nv * c.ss}
    if c.op != "encode":
        a.update(present=c.batch * n, err_log=c.batch * n * 2, out=c.batch * c.os)
    return a


def static_counts(c):
    """(units that run a second tile, units that run a third) under the static
    schedule, from T tiles over `units` workgroups (waves)"""
    grid = min(c.T, c.units)
    if c.sched in ("stride", "adjacent", "grid_y"):  # unit u (adjacent: wave u % 8 of workgroup u / 8) starts at
        runs = [-(-(c.T - u) // grid) for u in range(grid)]  # tile u and steps by the grid
    elif c.sched == "range":
        per = -(-c.T // grid)
        runs = [max(0, min(per * (w + 1), c.T) - per * w) for w in range(grid)]
    else:
        assert c.sched == "spans"
        runs = []
        for lo, hi in span_ranges(c.T, grid):  # span x: the grid / 8 workgroups b % 8 == x, from lo + b / 8
            runs += [-(-(hi - lo - j) // (grid // SPANS)) for j in range(grid // SPANS)]
    return sum(r >= 2 for r in runs), sum(r >= 3 for r in runs)


def query(c, base=0x7F00_0000_0000):
    """the kernel name(s) the host-only queries give for the case, at made-up
    256-B-aligned buffer addresses (the payloads at their base offset)"""
    n, k, _ = E.code_params(c.nv)
    sl = E.shard_len(c.nv, c.plen)
    pay, sh, pr, el, out = (base + (i << 40) for i in range(5))
    enc = E.encode_kernel(c.nv, pay + c.off, c.plen, c.ps, c.batch, sh, c.ss)
    rec = E.reconstruct_kernel(c.nv, sh, sl, c.ss, pr, el, c.batch, out, c.os)
    if c.op == "generic":
        return enc, rec, E.systematic_kernel(c.nv, sh, sl, c.ss, c.batch, out, c.os)
    return enc if c.op == "encode" else rec
