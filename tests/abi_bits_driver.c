/* abi_bits_driver.c -- plain-C consumer of the bit-packed entries of include/ldpc_mi355x.h (compiled by
 * tests/test_bit_io_cpu.py with gcc -std=c99 -Wall -Werror and linked against libldpc_mi355x.so).  Without arguments:
 * the argument checks that need no device.  argv[1] = "gpu": a small irregular code decoded through
 * ldpc_bp_decode_batch_bits at bit offsets inside words, against ldpc_bp_decode_batch on the same syndromes. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ldpc_mi355x.h"

#define MS 47
#define MN 95
#define MB 333
#define SBIT0 77
#define EBIT0 129

static int get_bit(const uint64_t *w, int64_t k) { return (int)((w[k >> 6] >> (k & 63)) & 1u); }
static void put_bit(uint64_t *w, int64_t k, int v)
{
    w[k >> 6] = (w[k >> 6] & ~((uint64_t)1 << (k & 63))) | ((uint64_t)(v & 1) << (k & 63));
}

static int gpu_main(void)
{
    static int64_t colptr[MN + 1], rowval[3 * MN];
    static uint8_t syn[MB * MS], r_err[MB * MN], r_conv[MB], conv[MB];
    static int32_t r_it[MB], it[MB];
    static double r_llr[MB * MN], llr[MB * MN];
    /* word vectors with room before and after the ranges */
    static uint64_t syn_w[(SBIT0 + MB * MS) / 64 + 3], err_w[(EBIT0 + MB * MN) / 64 + 3], pattern[(EBIT0 + MB * MN) / 64 + 3];
    const int64_t n_err_w = (int64_t)(sizeof err_w / sizeof err_w[0]);
    int64_t nnz = 0;
    uint32_t lcg = 2024u;
    ldpc_bp_decoder *dec = NULL;
    for (int j = 0; j < MN; ++j) {
        int64_t r[3] = {j % MS, (5 * j + 7) % MS, (11 * j + 3) % MS};
        colptr[j] = nnz;
        for (int a = 0; a < 3; ++a) for (int b = a + 1; b < 3; ++b) if (r[b] < r[a]) { int64_t q = r[a]; r[a] = r[b]; r[b] = q; }
        for (int a = 0; a < 3; ++a) if (a == 0 || r[a] != r[a - 1]) rowval[nnz++] = r[a];
    }
    colptr[MN] = nnz;
    memset(syn, 0, sizeof syn);
    for (int b = 0; b < MB; ++b)
        for (int j = 0; j < MN; ++j) {
            lcg = lcg * 1664525u + 1013904223u;
            if ((lcg >> 8) % 100u < (unsigned)(b % 9))
                for (int64_t k = colptr[j]; k < colptr[j + 1]; ++k) syn[b * MS + rowval[k]] ^= 1;
        }
    if (ldpc_bp_create(MS, MN, nnz, colptr, rowval, 0.04, 20, NULL, &dec) != LDPC_OK) { fprintf(stderr, "create: %s\n", ldpc_last_error()); return 30; }
    if (ldpc_bp_decode_batch(dec, MB, syn, r_err, r_conv, r_llr, r_it) != LDPC_OK) { fprintf(stderr, "byte entry: %s\n", ldpc_last_error()); return 31; }
    for (size_t q = 0; q < sizeof syn_w / sizeof syn_w[0]; ++q) { lcg = lcg * 1664525u + 1013904223u; syn_w[q] = ((uint64_t)lcg << 32) ^ (lcg * 2654435761u); }
    for (int64_t q = 0; q < n_err_w; ++q) { lcg = lcg * 1664525u + 1013904223u; pattern[q] = err_w[q] = ((uint64_t)lcg << 32) ^ (lcg * 40503u); }
    for (int64_t k = 0; k < (int64_t)MB * MS; ++k) put_bit(syn_w, SBIT0 + k, syn[k]);
    memset(conv, 9, sizeof conv);
    if (ldpc_bp_decode_batch_bits(dec, MB, syn_w, SBIT0, err_w, EBIT0, conv, llr, it) != LDPC_OK) { fprintf(stderr, "bits entry: %s\n", ldpc_last_error()); return 32; }
    for (int64_t k = 0; k < 64 * n_err_w; ++k) {
        const int inside = k >= EBIT0 && k < EBIT0 + (int64_t)MB * MN;
        const int want = inside ? r_err[k - EBIT0] : get_bit(pattern, k);
        if (get_bit(err_w, k) != want) { fprintf(stderr, "bit %ld (%s the range) differs\n", (long)k, inside ? "inside" : "outside"); return 33; }
    }
    if (memcmp(conv, r_conv, sizeof conv) || memcmp(it, r_it, sizeof it) || memcmp(llr, r_llr, sizeof llr)) return 34;
    {
        int nconv = 0;
        for (int b = 0; b < MB; ++b) nconv += r_conv[b];
        if (nconv < MB / 10 || nconv > MB - MB / 10) { fprintf(stderr, "test batch is not mixed (%d converged)\n", nconv); return 35; }
    }
    ldpc_bp_destroy(dec);
    printf("abi_bits_driver gpu ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    uint64_t words[4] = {0, 0, 0, 0};
    uint8_t conv[4] = {0, 0, 0, 0};
    if (ldpc_abi_version() != LDPC_MI355X_ABI_VERSION) return 10;
    if (argc > 1 && strcmp(argv[1], "gpu") == 0) return gpu_main();
    /* refused on the arguments alone: no handle is needed, no device is touched */
    if (ldpc_bp_decode_batch_bits(NULL, 1, words, 0, words, 0, conv, NULL, NULL) != LDPC_ERR_INVALID_ARGUMENT) return 11;
    if (strlen(ldpc_last_error()) == 0) return 12;
    if (ldpc_bp_decode_batch_bits(NULL, -1, words, 0, words, 0, conv, NULL, NULL) != LDPC_ERR_INVALID_ARGUMENT) return 13;
    if (ldpc_bp_decode_batch_bits(NULL, 1, words, -1, words, 0, conv, NULL, NULL) != LDPC_ERR_INVALID_ARGUMENT) return 14;
    if (ldpc_bp_decode_batch_bits(NULL, 1, words, 0, words, -64, conv, NULL, NULL) != LDPC_ERR_INVALID_ARGUMENT) return 15;
    if (ldpc_bp_decode_batch_bits_device(NULL, 1, words, 0, words, 0, conv, NULL, NULL, NULL) != LDPC_ERR_INVALID_ARGUMENT) return 16;
    if (ldpc_bp_decode_batch_bits_device(NULL, -1, words, 0, words, 0, conv, NULL, NULL, NULL) != LDPC_ERR_INVALID_ARGUMENT) return 17;
    if (ldpc_bp_decode_batch_bits_device(NULL, 1, words, 0, words, -1, conv, NULL, NULL, NULL) != LDPC_ERR_INVALID_ARGUMENT) return 18;
    if (ldpc_bp_decode_batch_multi_bits(NULL, 1, words, 0, words, 0, conv, NULL, NULL) != LDPC_ERR_INVALID_ARGUMENT) return 19;
    if (ldpc_bp_decode_batch_multi_bits(NULL, -1, words, 0, words, 0, conv, NULL, NULL) != LDPC_ERR_INVALID_ARGUMENT) return 20;
    if (ldpc_bp_decode_batch_multi_bits(NULL, 1, words, -5, words, 0, conv, NULL, NULL) != LDPC_ERR_INVALID_ARGUMENT) return 21;
    printf("abi_bits_driver ok\n");
    return 0;
}
