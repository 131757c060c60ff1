"""The product kernels whose body is shared keep it in more files: the ones
with a ragged form (csrc/enc_k256w_body.hpp + enc_k256w_tile.inc,
dec_n1024x_body.hpp + dec_n1024x_tile.inc), and the two n = 1024 reconstruct
kernels' common phases (dec_n1024_dfft.inc + dec_n1024_store.inc, included by
dec_n1024.hip and, nested, by dec_n1024x_tile.inc: they come after it, the
substitution runs in order).  The variant generators patch ONE source by exact
string match and write ONE file, so they work on the flattened source: the
.hip with those includes replaced by the files' text."""
ROOT = __file__.rsplit("/scripts/", 1)[0]
CS = f"{ROOT}/erasure-coding-crust_amd/csrc"
BODIES = ("enc_k256w_body.hpp", "enc_k256w_tile.inc", "dec_n1024x_body.hpp", "dec_n1024x_tile.inc",
          "dec_n1024_dfft.inc", "dec_n1024_store.inc")


def flat(name):
    s = open(f"{CS}/{name}").read()
    for b in BODIES:
        inc = f'#include "{b}"\n'
        if inc in s:
            s = s.replace(inc, open(f"{CS}/{b}").read().replace("#pragma once\n", ""))
    return s
