/* Plain-C host of the ldpc_bitflip_* entries of include/ldpc_mi355x.h (built and run by tests/test_bitflip_cpu.py and
 * tests/test_gpu_bitflip.py).
 *   no argument:            links, validates arguments (no device needed), prints "cpu ok"
 *   gpu SEED B b0 b1 ...:   decodes on the GPU: the hand-checked cases of the 3 x 3 all-ones H, then B columns of the
 *                           syndrome (1, 1, 1) under LDPC_BF_TIE_RANDOM with SEED and column0 = 5 -- every vote is +3 in
 *                           iteration 1, so column i flips exactly one bit, which must be b_i (the caller's model says
 *                           which); prints "gpu ok" */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ldpc_mi355x.h"

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, "line %d: %s failed (%s)\n", __LINE__, #cond, ldpc_last_error()); \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

static const int64_t colptr[4] = {0, 3, 6, 9};
static const int64_t rowval[9] = {0, 1, 2, 0, 1, 2, 0, 1, 2};

static int cpu_leg(void)
{
    ldpc_bitflip_decoder *dec = NULL;
    ldpc_bitflip_options opt;
    const int64_t bad_rows[9] = {1, 0, 2, 0, 1, 2, 0, 1, 2};
    uint8_t buf[16] = {0};
    memset(&opt, 0, sizeof opt);
    opt.device = -1;
    CHECK(sizeof(ldpc_bitflip_options) == 64);
    CHECK(ldpc_abi_version() == LDPC_MI355X_ABI_VERSION);
    CHECK(ldpc_bitflip_create(3, 3, 9, colptr, bad_rows, 0.01, 10, NULL, &dec) == LDPC_ERR_INVALID_ARGUMENT && !dec);
    CHECK(ldpc_bitflip_create(3, 3, 8, colptr, rowval, 0.01, 10, NULL, &dec) == LDPC_ERR_INVALID_ARGUMENT && !dec);
    CHECK(ldpc_bitflip_create(3, 3, 9, colptr, rowval, 0.01, 10, NULL, NULL) == LDPC_ERR_INVALID_ARGUMENT);
    opt.tie_break = 3;
    CHECK(ldpc_bitflip_create(3, 3, 9, colptr, rowval, 0.01, 10, &opt, &dec) == LDPC_ERR_INVALID_ARGUMENT && !dec);
    opt.tie_break = LDPC_BF_TIE_LAST;
    if (ldpc_device_count() == 0)
        CHECK(ldpc_bitflip_create(3, 3, 9, colptr, rowval, 0.01, 10, &opt, &dec) == LDPC_ERR_NO_DEVICE && !dec);
    CHECK(ldpc_bitflip_decode_batch(NULL, 1, 0, buf, buf, buf, NULL, NULL) == LDPC_ERR_INVALID_ARGUMENT);
    CHECK(ldpc_bitflip_decode_batch_device(NULL, 1, 0, buf, buf, buf, NULL, NULL, NULL) == LDPC_ERR_INVALID_ARGUMENT);
    CHECK(ldpc_bitflip_kernel(NULL) == 0 && ldpc_bitflip_destroy(NULL) == LDPC_OK);
    printf("cpu ok\n");
    return 0;
}

static int gpu_leg(int argc, char **argv)
{
    ldpc_bitflip_decoder *dec = NULL;
    ldpc_bitflip_options opt;
    /* (1,0,0): every vote -1 -> reason 2; (1,1,1): FIRST flips bit 0 and matches in iteration 2; zeros: matched at once;
       (2,1,1): check 0 never matches, the votes stay >= 0, bit 0 is toggled in each of the 10 iterations */
    const uint8_t syn[12] = {1, 0, 0, 1, 1, 1, 0, 0, 0, 2, 1, 1};
    uint8_t err[12], conv[4], stop[4];
    int32_t iters[4];
    const uint64_t seed = strtoull(argv[2], NULL, 10);
    const int B = atoi(argv[3]);
    int i;
    CHECK(argc == 4 + B && B > 0 && B <= 64);
    memset(&opt, 0, sizeof opt);
    opt.device = -1;
    opt.tie_break = LDPC_BF_TIE_FIRST;
    CHECK(ldpc_bitflip_create(3, 3, 9, colptr, rowval, 0.01, 10, &opt, &dec) == LDPC_OK && dec);
    CHECK(ldpc_bitflip_kernel(dec) == 1);
    CHECK(ldpc_bitflip_decode_batch(dec, 4, -1, syn, err, conv, iters, stop) == LDPC_ERR_INVALID_ARGUMENT);
    memset(err, 7, sizeof err);
    CHECK(ldpc_bitflip_decode_batch(dec, 4, 0, syn, err, conv, iters, stop) == LDPC_OK);
    CHECK(err[0] == 0 && err[1] == 0 && err[2] == 0 && conv[0] == 1 && iters[0] == 1 && stop[0] == 2);
    CHECK(err[3] == 1 && err[4] == 0 && err[5] == 0 && conv[1] == 1 && iters[1] == 2 && stop[1] == 1);
    CHECK(err[6] == 0 && err[7] == 0 && err[8] == 0 && conv[2] == 1 && iters[2] == 1 && stop[2] == 1);
    CHECK(err[9] == 0 && err[10] == 0 && err[11] == 0 && conv[3] == 0 && iters[3] == 10 && stop[3] == 0);
    CHECK(ldpc_bitflip_decode_batch(dec, 4, 0, syn, err, conv, NULL, NULL) == LDPC_OK && err[3] == 1);   /* optional outputs */
    CHECK(ldpc_bitflip_destroy(dec) == LDPC_OK);
    {
        uint8_t *s1 = malloc(3 * (size_t)B), *e1 = malloc(3 * (size_t)B), *c1 = malloc((size_t)B);
        CHECK(s1 && e1 && c1);
        memset(s1, 1, 3 * (size_t)B);
        opt.tie_break = LDPC_BF_TIE_RANDOM;
        opt.seed = seed;
        CHECK(ldpc_bitflip_create(3, 3, 9, colptr, rowval, 0.01, 10, &opt, &dec) == LDPC_OK);
        CHECK(ldpc_bitflip_decode_batch(dec, B, 5, s1, e1, c1, NULL, NULL) == LDPC_OK);
        for (i = 0; i < B; ++i) {
            const int want = atoi(argv[4 + i]);
            CHECK(c1[i] == 1 && e1[3 * i] + e1[3 * i + 1] + e1[3 * i + 2] == 1 && e1[3 * i + want] == 1);
        }
        CHECK(ldpc_bitflip_destroy(dec) == LDPC_OK);
        free(s1); free(e1); free(c1);
    }
    printf("gpu ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 4 && strcmp(argv[1], "gpu") == 0) return gpu_leg(argc, argv);
    return cpu_leg();
}
