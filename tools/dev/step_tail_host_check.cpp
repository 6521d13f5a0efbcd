// Host side of csrc/step_tail.hip under AddressSanitizer + UBSan (tools/dev/step_tail_host_check.py builds and runs this): the size
// getters, and every entry point with arguments it must refuse before it touches the device -- null pointers, NL = 0, negative
// counts, misaligned tables.  Needs no GPU and must never reach one: a call that returned 0 here would have launched.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../include/mgnns_step.h"

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, mgnns_last_error()); \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

int main() {
    alignas(16) static double buf[64];
    float* f = reinterpret_cast<float*>(buf);
    const int64_t* t = reinterpret_cast<const int64_t*>(buf);
    char* bytes = reinterpret_cast<char*>(buf);

    EXPECT(mgnns_step_chunk_elems() == MGNNS_STEP_CHUNK && MGNNS_STEP_CHUNK % 4 == 0);
    EXPECT(mgnns_step_chunk_record_bytes() == 40);
    EXPECT(mgnns_step_chunk_table_bytes(3) == 120 && mgnns_step_chunk_table_bytes(0) == 0 && mgnns_step_chunk_table_bytes(-7) == 0);
    EXPECT(mgnns_step_chunk_table_bytes(2147483647) == 40ull * 2147483647ull);
    EXPECT(mgnns_step_group_table_bytes(2) == 2 * 4 * MGNNS_STEP_GROUP_FLOATS && mgnns_step_group_table_bytes(-1) == 0);
    EXPECT(mgnns_step_partials_bytes(5) == 40 && mgnns_step_partials_bytes(-2147483647 - 1) == 0);
    EXPECT(mgnns_step_partials_bytes(2147483647) == 8ull * 2147483647ull);

    EXPECT(mgnns_ce_loss_fwd_bwd(nullptr, t, 1, 3, f, f, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_ce_loss_fwd_bwd(f, nullptr, 1, 3, f, f, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_ce_loss_fwd_bwd(f, t, 1, 3, nullptr, f, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_ce_loss_fwd_bwd(f, t, 1, 3, f, nullptr, nullptr) == MGNNS_ERR_ARG);
    const int bad_shapes[][2] = {{1, 0}, {1, -1}, {1, MGNNS_CE_MAX_NL + 1}, {0, 3}, {-5, 3}, {-2147483647 - 1, 2147483647}};
    for (const auto& s : bad_shapes) {
        EXPECT(mgnns_ce_loss_fwd_bwd(f, t, s[0], s[1], f, f, nullptr) == MGNNS_ERR_UNSUPP);
        EXPECT(strstr(mgnns_last_error(), "NL") != nullptr);
    }

    EXPECT(mgnns_grad_sumsq(buf, -1, buf, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_grad_sumsq(nullptr, 1, buf, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_grad_sumsq(buf, 1, nullptr, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_grad_sumsq(bytes + 4, 1, buf, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_grad_sumsq(buf, 1, reinterpret_cast<double*>(bytes + 4), nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_grad_sumsq(nullptr, 0, nullptr, nullptr) == 0);          // nothing to do is not an error, and launches nothing

    EXPECT(mgnns_grad_clip_coef(buf, -1, 1.0f, f, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_grad_clip_coef(nullptr, 1, 1.0f, f, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_grad_clip_coef(buf, 1, 1.0f, nullptr, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_grad_clip_coef(buf, 1, -1.0f, f, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_grad_clip_coef(buf, 1, NAN, f, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_grad_clip_coef(reinterpret_cast<const double*>(bytes + 4), 1, 1.0f, f, nullptr) == MGNNS_ERR_ARG);

    EXPECT(mgnns_adam_step(buf, -1, f, 1, f, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_adam_step(buf, 1, f, -1, f, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_adam_step(buf, 1, f, 0, f, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_adam_step(nullptr, 1, f, 1, f, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_adam_step(buf, 1, nullptr, 1, f, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_adam_step(buf, 1, f, 1, nullptr, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_adam_step(bytes + 4, 1, f, 1, f, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_adam_step(buf, 1, reinterpret_cast<const float*>(bytes + 2), 1, f, nullptr) == MGNNS_ERR_ARG);
    EXPECT(mgnns_adam_step(nullptr, 0, nullptr, 0, nullptr, nullptr) == 0);

    if (failures) {
        printf("%d checks FAILED\n", failures);
        return 1;
    }
    printf("clean: the size getters and every refused call, no sanitizer report\n");
    return 0;
}
