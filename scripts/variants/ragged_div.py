#!/usr/bin/env python3
"""Diagnostic variant of the ragged kernels' tile -> item lookup (DESIGN.md
§5.9): ragged_find_item's 64-ary search of tile_first replaced by the uniform
kernels' division, item = ticket / tiles per item.  Only right for a batch of
EQUAL items (scripts/bench_ragged.py's second measurement, --diag): it shows
what the search itself costs there.

  ragged_div.py OUT.hpp
Build: scripts/build_var.sh diag_ragged_div "" ragged.hpp=OUT.hpp"""
import sys

ROOT = __file__.rsplit("/scripts/", 1)[0]
s = open(f"{ROOT}/erasure-coding-crust_amd/csrc/ragged.hpp").read()
start = s.index("  uint32_t lo = 1, n = batch;  // the count of j")
end = s.index("  return uint32_t(__builtin_amdgcn_readfirstlane(int(lo - 1)));\n")
assert s.count("return uint32_t(__builtin_amdgcn_readfirstlane(int(lo - 1)));") == 1
s = (s[:start] + "  (void)batch;\n  (void)lane;\n  return t / tile_first[1];  // equal items: tiles per item\n" +
     s[end + len("  return uint32_t(__builtin_amdgcn_readfirstlane(int(lo - 1)));\n"):])
open(sys.argv[1], "w").write(s)
