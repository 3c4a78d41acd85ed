// Host-side sanitizer driver for the argument checks of cbw_align_matrix, cbw_dtw_dev and cbw_token_ts_ws_bytes (token-
// level timestamps on the GPU; include/cbw.h), beside host_driver.cpp and built the same way by tools/sanitize_host.sh:
// runtime.cpp under AddressSanitizer + UndefinedBehaviorSanitizer on its host side, no GPU.  Every call below is
// refused before any GPU work; the host pointers stand in for device memory and are never dereferenced.
#include <cstdint>
#include <cstdio>

#include "cbw.h"

static int failures = 0;
#define EXPECT(cond, what)                                                    \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "FAIL %s (%s:%d): %s\n", what, __FILE__, __LINE__, cbw_last_error()); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

int main() {
    float fm[4] = {0.f, 0.f, 0.f, 0.f};
    int32_t flag = 0, a = 0, ff[2] = {0, 0}, words[8] = {0};
    EXPECT(cbw_token_ts_ws_bytes(2, 2) == 8 && cbw_token_ts_ws_bytes(447, 1500) == 4 * 447 * 122, "token_ts_ws_bytes");
    EXPECT(cbw_token_ts_ws_bytes(0, 2) == -1 && cbw_token_ts_ws_bytes(1025, 2) == -1 &&
               cbw_token_ts_ws_bytes(2, 0) == -1 && cbw_token_ts_ws_bytes(2, 1501) == -1,
           "token_ts_ws_bytes refuses");
    EXPECT(cbw_align_matrix(nullptr, 1, 2, 0, 2, 2, 7, fm, &flag, words, 32, nullptr) == CBW_ERR_INVALID, "align_matrix null probs");
    EXPECT(cbw_align_matrix(fm, 1, 2, 0, 2, 2, 7, nullptr, &flag, words, 32, nullptr) == CBW_ERR_INVALID, "align_matrix null matrix");
    EXPECT(cbw_align_matrix(fm, 1, 2, 0, 2, 2, 7, fm, nullptr, words, 32, nullptr) == CBW_ERR_INVALID, "align_matrix null flag");
    EXPECT(cbw_align_matrix(fm, 0, 2, 0, 2, 2, 7, fm, &flag, words, 32, nullptr) == CBW_ERR_INVALID, "align_matrix n 0");
    EXPECT(cbw_align_matrix(fm, 1, 2, 0, 1, 2, 7, fm, &flag, words, 32, nullptr) == CBW_ERR_INVALID, "align_matrix T 1");
    EXPECT(cbw_align_matrix(fm, 1, 2, -1, 2, 2, 7, fm, &flag, words, 32, nullptr) == CBW_ERR_INVALID, "align_matrix t0 < 0");
    EXPECT(cbw_align_matrix(fm, 1, 2, 1, 2, 2, 7, fm, &flag, words, 32, nullptr) == CBW_ERR_INVALID, "align_matrix t0 + T > T_all");
    EXPECT(cbw_align_matrix(fm, 1, 2, 0, 2, 0, 7, fm, &flag, words, 32, nullptr) == CBW_ERR_INVALID, "align_matrix F 0");
    EXPECT(cbw_align_matrix(fm, 1, 2, 0, 2, 1501, 7, fm, &flag, words, 32, nullptr) == CBW_ERR_INVALID, "align_matrix F 1501");
    EXPECT(cbw_align_matrix(fm, 1, 2, 0, 2, 2, 4, fm, &flag, words, 32, nullptr) == CBW_ERR_INVALID, "align_matrix even width");
    EXPECT(cbw_align_matrix(fm, 1, 2, 0, 2, 2, 9, fm, &flag, words, 32, nullptr) == CBW_ERR_INVALID, "align_matrix width 9");
    EXPECT(cbw_align_matrix(fm, 1, 2, 0, 2, 2, 7, fm, &flag, words, 7, nullptr) == CBW_ERR_INVALID, "align_matrix small ws");
    EXPECT(cbw_align_matrix(fm, 1, 2, 0, 2, 2, 7, fm, &flag, nullptr, 32, nullptr) == CBW_ERR_INVALID, "align_matrix null ws");
    EXPECT(cbw_dtw_dev(nullptr, 2, 2, ff, nullptr, nullptr, nullptr, words, 32, nullptr) == CBW_ERR_INVALID, "dtw_dev null matrix");
    EXPECT(cbw_dtw_dev(fm, 2, 2, nullptr, nullptr, nullptr, nullptr, words, 32, nullptr) == CBW_ERR_INVALID, "dtw_dev null first_frame");
    EXPECT(cbw_dtw_dev(fm, 0, 2, ff, nullptr, nullptr, nullptr, words, 32, nullptr) == CBW_ERR_INVALID, "dtw_dev T 0");
    EXPECT(cbw_dtw_dev(fm, 1025, 2, ff, nullptr, nullptr, nullptr, words, 32, nullptr) == CBW_ERR_INVALID, "dtw_dev T 1025");
    EXPECT(cbw_dtw_dev(fm, 2, 0, ff, nullptr, nullptr, nullptr, words, 32, nullptr) == CBW_ERR_INVALID, "dtw_dev F 0");
    EXPECT(cbw_dtw_dev(fm, 2, 2, ff, &a, nullptr, nullptr, words, 32, nullptr) == CBW_ERR_INVALID, "dtw_dev path partly set");
    EXPECT(cbw_dtw_dev(fm, 2, 2, ff, nullptr, nullptr, nullptr, words, 7, nullptr) == CBW_ERR_INVALID, "dtw_dev small ws");
    EXPECT(cbw_dtw_dev(fm, 2, 2, ff, nullptr, nullptr, nullptr, nullptr, 32, nullptr) == CBW_ERR_INVALID, "dtw_dev null ws");
    if (failures) {
        std::fprintf(stderr, "%d token-timestamp argument checks failed\n", failures);
        return 1;
    }
    std::printf("token-timestamp argument checks passed\n");
    return 0;
}
