// host_pipe_plan_sanitize.cpp -- the HIP-free arithmetic of the BP host staging (csrc/host_pipe_plan.hpp: stage_layout,
// pipe_chunks, span_of, merge_bit_range) under AddressSanitizer + UBSan on the CPU.  The chunk rule against values worked
// out by hand from the rule in words (24 MiB / bytes per syndrome, floor, round up to 4096, no trailing chunk under half a
// chunk); the layout against the carving written out by hand; span_of + merge_bit_range against a bit-by-bit model with
// source and destination allocated at exactly the covering word count.  Built and run by
// tests/test_host_pipe_plan_cpu.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ldpcdecoders.jl_amd/csrc ...
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_pipe_plan.hpp"

using namespace ldpc_detail;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            return false;                                                         \
        }                                                                         \
    } while (0)

static uint64_t g_seed = 88172645463325252ull;
static uint64_t rnd()
{
    g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17;
    return g_seed;
}

static bool chunk_rule()
{
    auto is = [](ChunkPlan c, size_t cb, size_t nchunks) { return c.cb == cb && c.nchunks == nchunks; };
    // 24 MiB / 761 = 33069 -> 36864 (9 x 4096); 150001 = 4 x 36864 + 2545
    CHECK(is(pipe_chunks(761, 32768, 150001), 36864, 5));
    // 24 MiB / 4793 = 5250 -> the floor; 49151 < 1.5 x 32768 = 49152: one chunk of the whole batch, 49152 is two
    CHECK(is(pipe_chunks(4793, 32768, 49151), 49151, 1));
    CHECK(is(pipe_chunks(4793, 32768, 49152), 32768, 2));
    // the floor of the kernels that are not on-chip: 150001 = 2 x 65536 + 18929
    CHECK(is(pipe_chunks(761, 65536, 150001), 65536, 3));
    // above the floor: 24 MiB / 195 = 129055 -> 131072; 300000 = 2 x 131072 + 37856
    CHECK(is(pipe_chunks(195, 65536, 300000), 131072, 3));
    // 1 MiB chunks: 1377 syndromes -> the floor, and 40003 < 49152
    CHECK(is(pipe_chunks(761, 32768, 40003, 1), 40003, 1));
    CHECK(is(pipe_chunks(761, 32768, 40003, 0), 40003, 1));       // (a chunk size of 0 MiB counts as 1)
    // the override sets the chunk outright: 40003 = 4 x 9999 + 7; beyond the batch it is still one chunk
    CHECK(is(pipe_chunks(761, 32768, 40003, 24, 9999), 9999, 5));
    CHECK(is(pipe_chunks(761, 32768, 12001, 24, 20000), 20000, 1));
    CHECK(is(pipe_chunks(0, 32768, 1), 1, 1));                    // (an empty graph: no division by zero)
    return true;
}

// the image as the two entries carved it by hand: bytes, and the words covering bits
static size_t carved_by_hand(bool bits, size_t B, size_t s, size_t n, bool llr, size_t off[4])
{
    auto wbytes = [](size_t nbits) { return (((nbits + 63) >> 6) + 1) * sizeof(uint64_t); };
    Carve image;
    image.take(bits ? wbytes(B * s) : B * s);
    off[0] = image.take(bits ? wbytes(B * n) : B * n);
    off[1] = image.take(B);
    off[2] = image.take(B * sizeof(int32_t));
    off[3] = image.take(llr ? B * n * sizeof(double) : 0);
    return image.at;
}

static bool layout(int *count)
{
    // one syndrome of the s = 517, n = 1003 code: 517 -> 768, 1003 -> 1024, 1 -> 256, 4 -> 256, 8024 -> 8192
    StageLayout L = stage_layout(1, 517, 1003, false, 1003);
    CHECK(L.o_err == 768 && L.o_conv == 1792 && L.o_it == 2048 && L.o_llr == 2304 && L.total == 2304);
    L = stage_layout(1, 517, 1003, true, 1003);
    CHECK(L.o_llr == 2304 && L.total == 10496);
    for (size_t B : {(size_t)1, (size_t)63, (size_t)256, (size_t)3000, (size_t)12001, (size_t)36864, (size_t)49151})
        for (size_t s : {(size_t)0, (size_t)1, (size_t)252, (size_t)517})
            for (size_t n : {(size_t)0, (size_t)1, (size_t)504, (size_t)1003})
                for (int llr = 0; llr < 2; ++llr)
                    for (int bits = 0; bits < 2; ++bits) {
                        size_t off[4];
                        const size_t total = carved_by_hand(bits != 0, B, s, n, llr != 0, off);
                        L = bits ? stage_layout(B, word_image_bytes(B * s), word_image_bytes(B * n), llr != 0, n)
                                 : stage_layout(B, B * s, B * n, llr != 0, n);
                        ++*count;
                        CHECK(L.o_err == off[0] && L.o_conv == off[1] && L.o_it == off[2] && L.o_llr == off[3] && L.total == total);
                        CHECK(L.o_err <= L.o_conv && L.o_conv < L.o_it && L.o_it < L.o_llr && L.o_llr <= L.total);
                        CHECK(((L.o_err | L.o_conv | L.o_it | L.o_llr | L.total) & 255) == 0);
                        CHECK(L.o_err >= (bits ? word_image_bytes(B * s) : B * s) && L.o_conv - L.o_err >= (bits ? word_image_bytes(B * n) : B * n));
                        CHECK(L.o_it - L.o_conv >= B && L.o_llr - L.o_it >= 4 * B && L.total - L.o_llr >= (llr ? 8 * B * n : 0));
                    }
    // the ring-growth test of tests/test_gpu_bit_io.py (s = 517, n = 1003, 12001 syndromes): the whole batch is beyond the
    // 4 MiB of the small-batch round trip in every call, and the chunk images are small, in between, large
    const size_t small_limit = (size_t)4 << 20, s = 517, n = 1003;
    auto bytes_image = [&](size_t B) { return stage_layout(B, B * s, B * n, false, n).total; };
    CHECK(bytes_image(12001) > small_limit);
    CHECK(bytes_image(3000) < bytes_image(5000) && bytes_image(5000) < bytes_image(12001));
    CHECK(pipe_chunks(s + n + 5, 32768, 12001, 24, 12001).nchunks == 1 && pipe_chunks(s + n + 5, 32768, 12001, 24, 3000).nchunks == 5 &&
          pipe_chunks(s + n + 5, 32768, 12001, 24, 5000).nchunks == 3);
    CHECK(stage_layout(12001, word_image_bytes(12001 * s), word_image_bytes(12001 * n), false, n).total < small_limit);   // (hence with LLRs:)
    CHECK(stage_layout(12001, word_image_bytes(12001 * s), word_image_bytes(12001 * n), true, n).total > small_limit);
    CHECK(stage_layout(4000, word_image_bytes(4000 * s), word_image_bytes(4000 * n), true, n).total > bytes_image(12001));
    return true;
}

static bool get_bit(const std::vector<uint64_t> &w, size_t i) { return (w[i >> 6] >> (i & 63)) & 1; }

// every offset and length: bits inside the range come from src, guard bits stay
static bool merge_every_offset(int *count)
{
    for (int off = 0; off < 64; ++off)
        for (size_t len = 0; len <= 200; ++len)
            for (int own_copy = 0; own_copy < 2; ++own_copy) {
                const size_t nw = len ? ((size_t)off + len + 63) >> 6 : 0;
                std::vector<uint64_t> src(nw), dst(nw);
                for (auto &w : src) w = rnd();
                for (auto &w : dst) w = rnd();
                const std::vector<uint64_t> before = dst;
                size_t copied = 0;
                if (own_copy)
                    merge_bit_range(dst.data(), src.data(), off, len, [&](void *d, const void *s, size_t b) { std::memcpy(d, s, b); copied += b; });
                else
                    merge_bit_range(dst.data(), src.data(), off, len);
                for (size_t i = 0; i < nw * 64; ++i) {
                    const bool inside = i >= (size_t)off && i < (size_t)off + len;
                    CHECK(get_bit(dst, i) == (inside ? get_bit(src, i) : get_bit(before, i)));
                }
                if (own_copy) CHECK(copied % 8 == 0 && copied / 8 <= nw && copied / 8 + 2 >= nw);
                ++*count;
            }
    return true;
}

// a batch of B columns of r bits at bit0 of a caller's array, chunk by chunk as the pipeline does it: the image of a
// chunk holds exactly the covering words, the caller's array exactly the words covering [0, bit0 + B r)
static bool chunks_into_a_callers_array(int *count)
{
    for (int64_t bit0 : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)64, (int64_t)777})
        for (size_t r : {(size_t)1, (size_t)7, (size_t)64, (size_t)67, (size_t)129})
            for (size_t B : {(size_t)1, (size_t)5, (size_t)64, (size_t)101})
                for (size_t cb : {(size_t)1, (size_t)3, (size_t)64, (size_t)200}) {
                    const size_t nbits = (size_t)bit0 + B * r;
                    std::vector<uint64_t> arr((nbits + 63) >> 6), want_bits((nbits + 63) >> 6);
                    for (auto &w : arr) w = rnd();
                    for (auto &w : want_bits) w = rnd();
                    const std::vector<uint64_t> before = arr;
                    size_t covered = 0;
                    for (size_t b0 = 0; b0 < B; b0 += cb) {
                        const size_t nb = std::min(cb, B - b0);
                        const Span sp = span_of(bit0, b0, nb, r);
                        CHECK(sp.w0 * 64 + (size_t)sp.off == (size_t)bit0 + b0 * r && sp.off >= 0 && sp.off < 64);
                        CHECK(sp.nwords == (((size_t)sp.off + nb * r + 63) >> 6) && sp.w0 + sp.nwords <= arr.size());
                        CHECK(sp.nwords * 8 <= word_image_bytes(nb * r));
                        std::vector<uint64_t> image(sp.nwords);   // what the device leaves: the chunk's bits at sp.off, anything around them
                        for (auto &w : image) w = rnd();
                        for (size_t i = 0; i < nb * r; ++i) {
                            const size_t at = (size_t)sp.off + i, from = (size_t)bit0 + b0 * r + i;
                            image[at >> 6] = (image[at >> 6] & ~((uint64_t)1 << (at & 63))) | ((uint64_t)get_bit(want_bits, from) << (at & 63));
                        }
                        merge_bit_range(arr.data() + sp.w0, image.data(), sp.off, nb * r);
                        covered += nb * r;
                    }
                    CHECK(covered == B * r);
                    for (size_t i = 0; i < arr.size() * 64; ++i) {
                        const bool inside = i >= (size_t)bit0 && i < nbits;
                        CHECK(get_bit(arr, i) == (inside ? get_bit(want_bits, i) : get_bit(before, i)));
                    }
                    ++*count;
                }
    const Span none = span_of(5, 3, 0, 17);
    CHECK(none.nwords == 0);
    return true;
}

int main()
{
    int layouts = 0, merges = 0, batches = 0;
    if (!chunk_rule()) return 1;
    if (!layout(&layouts)) return 2;
    if (!merge_every_offset(&merges)) return 3;
    if (!chunks_into_a_callers_array(&batches)) return 4;
    std::printf("OK host pipe plan: %d layouts, %d merges, %d chunked batches\n", layouts, merges, batches);
    return 0;
}
