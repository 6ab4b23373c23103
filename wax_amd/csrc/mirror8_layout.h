// mirror8_layout.h — where the code of (row, element) sits in the 8-bit code mirror's buffer: THE definition, for the writer
// (mirror8_kernel), the reader (code8_pass) and the read-out (wax_hip_mirror8_snapshot). DESIGN 2, 4.1.
//
// The buffer is a sequence of 16-row tiles of 16 * D contiguous bytes, each in the order of the MFMA operand it becomes:
//   tile t = row >> 4, position p = row & 15;  element e = 64 s + 16 g + b  (k-step s, lane group g < 4, byte b < 16)
//   offset = t * 16 D  +  s * 1024  +  g * 256  +  p * 16  +  b
// so that lane l = 16 g + p of a wave finds its 16 bytes of k-step s at 1024 s + 16 l: one global_load_dwordx4 of the wave reads 1024
// contiguous bytes, eight whole 128-byte lines, instead of sixteen 64-byte halves of lines 384 bytes apart. Operand B (query_digits)
// relies on the elements a lane gets: 64 s + 16 (l >> 4) + [0, 16) of row l & 15 — checked below.
// A buffer of n rows holds ceil(n / 16) tiles; the {scale, err} words are not part of it (one float2 per row, row order).
// Plain C++14: the host compiler reads this header too (tests/test_mirror8_tiles_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WAX_MIRROR8_HD __host__ __device__
#else
#define WAX_MIRROR8_HD
#endif

namespace wax {

constexpr uint32_t MIRROR8_TILE_ROWS = 16;

// bytes of the buffer that holds `rows` rows: whole tiles
WAX_MIRROR8_HD constexpr size_t mirror8_bytes(uint64_t rows, uint32_t dims) {
    return (size_t)((rows + MIRROR8_TILE_ROWS - 1) / MIRROR8_TILE_ROWS) * MIRROR8_TILE_ROWS * dims;
}

// byte offset of the code of (row, element); dims a multiple of 64
WAX_MIRROR8_HD constexpr size_t mirror8_offset(uint64_t row, uint32_t element, uint32_t dims) {
    return (size_t)(row >> 4) * 16u * dims + (size_t)(element >> 6) * 1024u + (size_t)((element >> 4) & 3u) * 256u + (size_t)(row & 15u) * 16u +
           (element & 15u);
}

namespace mirror8_layout_check {

// lane l's 16 bytes of k-step s, at 1024 s + 16 l of the tile, are elements 64 s + 16 (l >> 4) + [0, 16) of row l & 15 — for every lane
// and k-step of a tile that is not the first, so that the tile term is checked too
constexpr bool lanes_hold_operand_a(uint32_t dims) {
    for (uint32_t s = 0; s < dims / 64; ++s)
        for (uint32_t l = 0; l < 64; ++l)
            for (uint32_t b = 0; b < 16; ++b)
                if (mirror8_offset(3 * 16 + (l & 15), 64 * s + 16 * (l >> 4) + b, dims) != (size_t)3 * 16 * dims + 1024 * s + 16 * l + b) return false;
    return true;
}

// every byte of [0, 16 D) is the offset of exactly one (row, element) of the tile. The lanes' slices above are disjoint 16-byte
// ranges that cover [0, 16 D) (s < D / 64, l < 64: 1024 s + 16 l + b), and every (row, element) of the tile is in exactly one slice —
// checked here by counting: 16 D pairs, all inside the tile, and the inverse map gives each pair back.
constexpr bool tile_is_bijection(uint32_t dims) {
    for (uint32_t off = 0; off < 16 * dims; ++off) {
        const uint32_t s = off >> 10, g = (off >> 8) & 3u, p = (off >> 4) & 15u, b = off & 15u;
        if (mirror8_offset(p, 64 * s + 16 * g + b, dims) != off) return false;       // onto: every offset is hit ...
    }
    for (uint32_t p = 0; p < 16; ++p)
        for (uint32_t e = 0; e < dims; ++e)
            if (mirror8_offset(p, e, dims) >= (size_t)16 * dims) return false;       // ... by 16 D pairs that all stay inside: one to one
    return true;
}

static_assert(lanes_hold_operand_a(384) && lanes_hold_operand_a(768), "a lane's load must hold the elements operand B holds");
static_assert(tile_is_bijection(384) && tile_is_bijection(768), "a tile's rows and elements fill [0, 16 D) exactly once");
static_assert(mirror8_offset(16, 0, 384) == 16 * 384 && mirror8_offset(33, 0, 768) == 2 * 16 * 768 + 16, "tiles are 16 D bytes apart");
static_assert(mirror8_bytes(0, 384) == 0 && mirror8_bytes(1, 384) == 16 * 384 && mirror8_bytes(17, 384) == 32 * 384, "whole tiles");

}  // namespace mirror8_layout_check

}  // namespace wax
