"""The product kernels whose body is shared with a ragged form keep it in two
more files (csrc/enc_k256w_body.hpp + enc_k256w_tile.inc, dec_n1024x_body.hpp +
dec_n1024x_tile.inc).  The variant generators patch ONE source by exact string
match and write ONE file, so they work on the flattened source: the .hip with
those includes replaced by the files' text."""
ROOT = __file__.rsplit("/scripts/", 1)[0]
CS = f"{ROOT}/erasure-coding-crust_amd/csrc"
BODIES = ("enc_k256w_body.hpp", "enc_k256w_tile.inc", "dec_n1024x_body.hpp", "dec_n1024x_tile.inc")


def flat(name):
    s = open(f"{CS}/{name}").read()
    for b in BODIES:
        inc = f'#include "{b}"\n'
        if inc in s:
            s = s.replace(inc, open(f"{CS}/{b}").read().replace("#pragma once\n", ""))
    return s
