// The DTW kernel of whisper_kernels.hip, compiled there twice: with DTW_BATCH 0 as dtw_kernel (one window, one
// workgroup; the text is then what the compiler saw before the batched launch existed, so that kernel keeps its
// code -- a body shared by inlining moved its register allocation), and with DTW_BATCH 1 as dtw_batch_kernel (N
// windows, workgroup blockIdx.x = window blockIdx.x of the table in the kernel arguments, the block sized for the
// largest T: a thread beyond its window's T takes part in every barrier and nothing else, each block runs its own
// window's steps; first_frame int32 [N][ld]; no path).
#if DTW_BATCH
__global__ __launch_bounds__(DTW_MAX_T) void dtw_batch_kernel(const cbw_ts_batch wins, int* __restrict__ first_frames,
                                                              int ld) {
    const float* __restrict__ m = wins.w[blockIdx.x].matrix;
    const int T = wins.w[blockIdx.x].T, F = wins.w[blockIdx.x].F;
    int* __restrict__ first_frame = first_frames + (int64_t)blockIdx.x * ld;
    uint32_t* __restrict__ trace = wins.w[blockIdx.x].trace;
    int* const text_idx = nullptr;
    int* const time_idx = nullptr;
    int* const len = nullptr;
#else
__global__ __launch_bounds__(DTW_MAX_T) void dtw_kernel(const float* __restrict__ m, int T, int F,
                                                        int* __restrict__ first_frame, int* __restrict__ text_idx,
                                                        int* __restrict__ time_idx, int* __restrict__ len,
                                                        uint32_t* __restrict__ trace) {
#endif
    __shared__ float sh[2][DTW_MAX_T];
    __shared__ int n_sh;
    const int i = threadIdx.x;
    const bool row = i < T;
    const float* __restrict__ mr = m + (int64_t)min(i, T - 1) * F;
    const int nblk = (T + F - 1 + 15) >> 4;
    float ma[16], mb[16];   // two blocks of matrix entries, used in turn: no copy between them
    dtw_load16(mr, -i, F, ma);
    float left = INFINITY, diag = i == 0 ? 0.f : INFINITY;
    for (int b = 0; b < nblk; b += 2) {
        dtw_load16(mr, 16 * (b + 1) - i, F, mb);
        const uint32_t wa = dtw_block16(ma, b, i, row, F, sh, left, diag);
        if (row) trace[(int64_t)b * T + i] = wa;
        if (b + 1 == nblk) break;
        dtw_load16(mr, 16 * (b + 2) - i, F, ma);
        const uint32_t wb = dtw_block16(mb, b + 1, i, row, F, sh, left, diag);
        if (row) trace[(int64_t)(b + 1) * T + i] = wb;
    }
    __syncthreads();   // the trace words of every wave are in memory
    if (i == 0) {
        int r = T, c = F, n = 0;   // 1-based, as cbw_dtw's tables: row 0 walks left, column 0 walks up
        int64_t at = -1;
        uint32_t word = 0;
        while (r > 0 || c > 0) {
            if (text_idx) {
                text_idx[n] = r - 1;
                time_idx[n] = c - 1;
            }
            ++n;
            uint32_t t;
            if (c == 0) t = 1;
            else if (r == 0) t = 2;
            else {
                const int d = r + c - 2;
                const int64_t idx = (int64_t)(d >> 4) * T + (r - 1);
                if (idx != at) word = trace[idx], at = idx;
                t = (word >> (2 * (d & 15))) & 3u;
            }
            if (t != 2) first_frame[r - 1] = c - 1, --r;
            if (t != 1) --c;
        }
        n_sh = n;
        if (len) *len = n;
    }
    __syncthreads();
    if (text_idx) {
        const int n = n_sh;
        for (int k = i; k < n / 2; k += blockDim.x) {
            const int a = text_idx[k], b = text_idx[n - 1 - k];
            text_idx[k] = b, text_idx[n - 1 - k] = a;
            const int p = time_idx[k], q = time_idx[n - 1 - k];
            time_idx[k] = q, time_idx[n - 1 - k] = p;
        }
    }
}
