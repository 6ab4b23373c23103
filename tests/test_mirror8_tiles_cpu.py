"""The storage order of the 8-bit code mirror (wax_amd/csrc/mirror8_layout.h) on the host: the header's own
static_asserts (a tile is a bijection onto [0, 16 D), a lane's 16 bytes are the elements operand B holds) fire when the consumer below
is compiled, and the offsets it prints for three tiles are compared with the formula restated here:

    offset(row, e) = (row >> 4) * 16 D + (e >> 6) * 1024 + ((e >> 4) & 3) * 256 + (row & 15) * 16 + (e & 15)
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 3 * 16

CONSUMER = r'''
#include <cstdio>
#include <cstdlib>
#include "mirror8_layout.h"
int main(int argc, char** argv) {
    const unsigned dims = (unsigned)std::atoi(argv[argc - 1]);
    for (unsigned r = 0; r < 48; ++r)
        for (unsigned e = 0; e < dims; ++e) std::printf("%zu\n", wax::mirror8_offset(r, e, dims));
    std::printf("%zu %zu %zu\n", wax::mirror8_bytes(0, dims), wax::mirror8_bytes(33, dims), wax::mirror8_bytes(48, dims));
    return 0;
}
'''


def offsets(rows, dims):
    r = np.arange(rows, dtype=np.int64)[:, None]
    e = np.arange(dims, dtype=np.int64)[None, :]
    return (r >> 4) * 16 * dims + (e >> 6) * 1024 + ((e >> 4) & 3) * 256 + (r & 15) * 16 + (e & 15)


@pytest.fixture(scope="module")
def consumer(tmp_path_factory):
    d = tmp_path_factory.mktemp("mirror8_layout")
    src, exe = d / "consumer.cpp", d / "consumer"
    src.write_text(CONSUMER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "wax_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    return str(exe)


@pytest.mark.parametrize("dims", [384, 768])
def test_the_header_places_every_code_where_the_formula_does(consumer, dims):
    out = subprocess.run([consumer, str(dims)], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
    got = np.array(out[:ROWS * dims], dtype=np.int64).reshape(ROWS, dims)
    want = offsets(ROWS, dims)
    assert np.array_equal(got, want), f"first difference at (row, element) {np.argwhere(got != want)[0]}"
    assert [int(v) for v in out[ROWS * dims].split()] == [0, 48 * dims, 48 * dims], "a buffer holds whole tiles"


@pytest.mark.parametrize("dims", [384, 768])
def test_the_formula_is_the_operand_order(dims):
    """What the static_asserts say, on the restated formula: three tiles fill [0, 48 D) exactly once, tile by tile, and lane l's
    16 bytes of k-step s (bytes 1024 s + 16 l of a tile) are elements 64 s + 16 (l >> 4) + [0, 16) of row l & 15."""
    off = offsets(ROWS, dims)
    assert np.array_equal(np.sort(off.ravel()), np.arange(ROWS * dims))
    for t in range(3):
        tile = off[16 * t:16 * t + 16]
        assert tile.min() == t * 16 * dims and tile.max() == (t + 1) * 16 * dims - 1
        for s in range(dims // 64):
            for lane in range(64):
                e0 = 64 * s + 16 * (lane >> 4)
                assert np.array_equal(tile[lane & 15, e0:e0 + 16], t * 16 * dims + 1024 * s + 16 * lane + np.arange(16))
