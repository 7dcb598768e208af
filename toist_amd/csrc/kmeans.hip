// Device-resident k-means for the noun-pronoun distillation step (BASELINE configs[4]).
//
// Replaces models/kmeans.py:21-96 as ClusterCriterion.memory_cluster calls it (/root/reference/models/mdetr.py:213-234): per
// sample, Lloyd iterations over the task's memory bank ([1024, 256] fp32) from the task's current centres (K = 3) until
// (sum_k |c_k' - c_k|)^2 < tol, the centres are stored back, and the centre nearest to the sample's own feature is picked.  The
// reference (and round 1 here) reads the shift back to the host after EVERY iteration; here the whole loop runs inside one
// workgroup -- one workgroup per distinct task of the batch, walking that task's samples in batch order so that a later sample
// starts from the centres the earlier one left, exactly like the sequential reference -- and the host never looks.
// Work per iteration: two passes over the 1 MB bank (L2-resident) = ~20 us on one CU by its bytes; neither roofline applies to 1-8 workgroups, and
// the sweep's launch below measures about 200 us per iteration (profiles/sweep_choice.json); more loads in flight per lane did not change that.
//
// The prototype choice of a task sweep (toist_sweep_prototypes) runs the same iterations and the same pick per (image, caption) pair, with the
// feature and the substitution into the encoder's bf16 rows in the same launch; lloyd_iterations / nearest_centre are what the entry points share.
//
// The same file holds what lets ONE captured graph serve a run from its first step: the start of models/kmeans.py:8-18 while a bank fills (the host
// draws the rows, the device's own full_label decides whether they are used: toist_kmeans_init) and the FIFO branch of the bank update with its
// update_count / full_label bookkeeping (mdetr.py:85-97: toist_bank_fifo), next to the masked row scatter of the nearest-replacement branch.
#include "common.h"

namespace toist {

constexpr int KM_THREADS = 1024, KM_MAXK = 8, KM_MAXD = 256;

constexpr int KM_START_MISMATCH = 1;   // status bit: full_label[task] and init_rows[sample] disagree about the start (toist_kmeans_init)

// The Lloyd iterations of one member, shared by every entry point of this file: from the centres in c[] until (sum_k |c_k' - c_k|)^2 < tol or max_iter,
// over the bank X [N, D].  The LDS arrays are the caller's (one set per kernel); every thread of the workgroup calls it and gets the iteration count.
__device__ __forceinline__ int lloyd_iterations(const float* __restrict__ X, int N, int D, int K, float tol, int max_iter, float (*c)[KM_MAXD],
                                                float (*part)[KM_MAXK][KM_MAXD], int (*cnt_part)[KM_MAXK], float* red, float* shift_sh_p,
                                                unsigned char* choice) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d_of = tid & 255, quarter = tid >> 8;  // update pass: thread = (feature, quarter of the points); needs D <= 256
    int it = 0;
    for (; it < max_iter; ++it) {
        // ---- assignment: one wavefront per point, lanes across the features ----
        for (int n = wave; n < N; n += KM_THREADS / 64) {
            float dist[KM_MAXK];
#pragma unroll
            for (int kk = 0; kk < KM_MAXK; ++kk) dist[kk] = 0.f;
            for (int d = lane; d < D; d += 64) {
                const float x = X[(long long)n * D + d];
#pragma unroll
                for (int kk = 0; kk < KM_MAXK; ++kk)
                    if (kk < K) { const float t = x - c[kk][d]; dist[kk] += t * t; }
            }
            int best = 0;
            float bd = 0.f;
#pragma unroll
            for (int kk = 0; kk < KM_MAXK; ++kk) {
                if (kk < K) {
                    const float v = wave_sum(dist[kk]);
                    if (kk == 0 || v < bd) { bd = v; best = kk; }      // first minimum wins, like torch.argmin
                }
            }
            if (lane == 0) choice[n] = (unsigned char)best;
        }
        __syncthreads();
        // ---- update: member sums per (cluster, feature), four quarters of the points in parallel ----
        {
            float s[KM_MAXK];
            int cn[KM_MAXK];
#pragma unroll
            for (int kk = 0; kk < KM_MAXK; ++kk) { s[kk] = 0.f; cn[kk] = 0; }
            const int per = (N + 3) / 4, n0 = quarter * per, n1 = min(N, n0 + per);
            if (d_of < D) {
                for (int n = n0; n < n1; ++n) {
                    const int ch = choice[n];
                    const float x = X[(long long)n * D + d_of];
#pragma unroll
                    for (int kk = 0; kk < KM_MAXK; ++kk)
                        if (kk == ch) { s[kk] += x; ++cn[kk]; }
                }
#pragma unroll
                for (int kk = 0; kk < KM_MAXK; ++kk)
                    if (kk < K) { part[quarter][kk][d_of] = s[kk]; if (d_of == 0) cnt_part[quarter][kk] = cn[kk]; }
            }
        }
        __syncthreads();
        // threads 0 .. K*D-1 finish one (cluster, feature) each; the squared moves go back to LDS for the per-cluster norms
        float nw = 0.f, df = 0.f;
        int fk = 0, fd = 0;
        if (tid < K * D) {
            fk = tid / D; fd = tid - fk * D;
            const int count = cnt_part[0][fk] + cnt_part[1][fk] + cnt_part[2][fk] + cnt_part[3][fk];
            const float old = c[fk][fd];
            nw = old;                                             // an empty cluster keeps its centre (kmeans.py:72)
            if (count > 0) nw = (((part[0][fk][fd] + part[1][fk][fd]) + part[2][fk][fd]) + part[3][fk][fd]) / (float)count;
            df = (nw - old) * (nw - old);
        }
        __syncthreads();                                          // every read of part[] is done
        if (tid < K * D) { c[fk][fd] = nw; part[0][fk][fd] = df; }
        __syncthreads();
        if (tid < K) {                                            // |c_k' - c_k| per cluster (D <= 256 terms)
            float t = 0.f;
            for (int d = 0; d < D; ++d) t += part[0][tid][d];
            red[tid] = sqrtf(t);
        }
        __syncthreads();
        if (tid == 0) {
            float sh = 0.f;
            for (int kk = 0; kk < K; ++kk) sh += red[kk];
            *shift_sh_p = sh;
        }
        __syncthreads();
        if (*shift_sh_p * *shift_sh_p < tol) { ++it; break; }
    }
    return it;
}

// The centre nearest to the feature row f [D] (first minimum wins): one wavefront, lanes across the features; every lane gets the index.
__device__ __forceinline__ int nearest_centre(const float* f, const float (*c)[KM_MAXD], int D, int K, int lane) {
    int best = 0;
    float bd = 0.f;
    for (int kk = 0; kk < K; ++kk) {
        float t = 0.f;
        for (int d = lane; d < D; d += 64) { const float u = f[d] - c[kk][d]; t += u * u; }
        t = wave_sum(t);
        if (kk == 0 || t < bd) { bd = t; best = kk; }
    }
    return best;
}

// The Lloyd body of both entry points.  START = false: every member starts from the centres in LDS (the stored ones, or what the previous member of
// the same task left).  START = true: the device's own full_label[task] decides -- 0 and init_rows[sample][0] >= 0: the centres are the bank rows
// init_rows[sample][0..K) (models/kmeans.py:8-18 with the host's np.random.choice draw), for every member anew; 1 and a negative row: as START =
// false; anything else: as START = false, and KM_START_MISMATCH is set in *status.
template <bool START>
__device__ __forceinline__ void kmeans_body(const float* __restrict__ banks, long long bank_stride, float* __restrict__ centers_all,
                                            long long centers_stride, const int* __restrict__ group_task,
                                            const int* __restrict__ group_off, const int* __restrict__ members,
                                            const float* __restrict__ features, int N, int D, int K, float tol, int max_iter,
                                            int* __restrict__ pick_out, float* __restrict__ center_out, int* __restrict__ iters_out,
                                            const float* __restrict__ full_label, const int* __restrict__ init_rows, int* __restrict__ status) {
    __shared__ float c[KM_MAXK][KM_MAXD];            // current centres
    __shared__ float part[4][KM_MAXK][KM_MAXD];      // per-quarter member sums
    __shared__ int cnt_part[4][KM_MAXK];
    __shared__ float red[KM_THREADS / 64];
    __shared__ float shift_sh;
    extern __shared__ unsigned char choice[];        // [N]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x, task = group_task[g];
    const float* X = banks + (long long)task * bank_stride;
    float* cg = centers_all + (long long)task * centers_stride;
    for (int i = tid; i < K * D; i += KM_THREADS) c[i / D][i % D] = cg[i];
    __syncthreads();
    for (int mi = group_off[g]; mi < group_off[g + 1]; ++mi) {
        const int sample = members[mi];
        if constexpr (START) {
            const int* row = init_rows + (long long)sample * K;
            const bool filling = full_label[task] == 0.f, drawn = row[0] >= 0;
            bool use = filling && drawn;
            for (int kk = 0; kk < K; ++kk) use = use && row[kk] >= 0 && row[kk] < N;     // (a row outside the bank is a mismatch too, never an address)
            if (use) {
                for (int i = tid; i < K * D; i += KM_THREADS) c[i / D][i % D] = X[(long long)row[i / D] * D + i % D];
                __syncthreads();
            } else if (filling || drawn) {
                if (tid == 0) atomicOr(status, KM_START_MISMATCH);
            }
        }
        const int it = lloyd_iterations(X, N, D, K, tol, max_iter, c, part, cnt_part, red, &shift_sh, choice);
        // ---- centres back to the task's slot; pick the centre nearest to this sample's feature ----
        for (int i = tid; i < K * D; i += KM_THREADS) cg[i] = c[i / D][i % D];
        if (wave == 0) {
            const int best = nearest_centre(features + (long long)sample * D, c, D, K, lane);
            if (lane == 0) { pick_out[sample] = best; if (iters_out) iters_out[sample] = it; }
            for (int d = lane; d < D; d += 64) center_out[(long long)sample * D + d] = c[best][d];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_kernel(const float* __restrict__ banks, long long bank_stride, float* __restrict__ centers_all,
                                                            long long centers_stride, const int* __restrict__ group_task,
                                                            const int* __restrict__ group_off, const int* __restrict__ members,
                                                            const float* __restrict__ features, int N, int D, int K, float tol, int max_iter,
                                                            int* __restrict__ pick_out, float* __restrict__ center_out, int* __restrict__ iters_out) {
    kmeans_body<false>(banks, bank_stride, centers_all, centers_stride, group_task, group_off, members, features, N, D, K, tol, max_iter, pick_out, center_out,
                       iters_out, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_init_kernel(const float* __restrict__ banks, long long bank_stride, float* __restrict__ centers_all,
                                                                 long long centers_stride, const int* __restrict__ group_task,
                                                                 const int* __restrict__ group_off, const int* __restrict__ members,
                                                                 const float* __restrict__ features, int N, int D, int K, float tol, int max_iter,
                                                                 int* __restrict__ pick_out, float* __restrict__ center_out, int* __restrict__ iters_out,
                                                                 const float* __restrict__ full_label, const int* __restrict__ init_rows,
                                                                 int* __restrict__ status) {
    kmeans_body<true>(banks, bank_stride, centers_all, centers_stride, group_task, group_off, members, features, N, D, K, tol, max_iter, pick_out, center_out,
                      iters_out, full_label, init_rows, status);
}

// ---- the prototype choice of a task sweep (mdetr.py:282-312 over the P (image, caption) pairs of toist_sweep_assemble), one launch ------------------
// One workgroup per group slot = per distinct task among the captions (unused slots exit).  The workgroup owns its task's centres in LDS and walks the
// pairs p = 0 .. live-1 in ascending order, serving those whose caption's task is its own: a later pair starts from the centres the earlier one left,
// the reference's sequential order; tasks share no state, so the grouping is exact.  Per served pair: the feature of the word 'something' (an fp32
// weighted sum over the L caption rows of the encoder's bf16 memory, every product formed and rounded, ascending l), kmeans_body<false>'s iterations
// and pick, the centres back to cluster_centers[task], and bf16(centre[pick]) into the marked caption rows of memory_mod -- nothing else of memory_mod,
// nothing of memory.  live and the tables are read from the device: the launch arguments do not depend on the batch.
constexpr int SP_MAXL = 256;

__global__ __launch_bounds__(KM_THREADS) void sweep_prototypes_kernel(const bf16_t* __restrict__ memory, bf16_t* __restrict__ memory_mod,
                                                                      const int* __restrict__ pair_caption, const int* __restrict__ live_p,
                                                                      const float* __restrict__ W_sth, const uint8_t* __restrict__ sub_sth,
                                                                      const int* __restrict__ cap_task, const int* __restrict__ group_task,
                                                                      const float* __restrict__ banks, long long bank_stride,
                                                                      float* __restrict__ centers_all, long long centers_stride, int P, int HW, int L,
                                                                      int T, int n_tasks, int N, int D, int K, float tol, int max_iter,
                                                                      int* __restrict__ status, int* __restrict__ pick_out,
                                                                      float* __restrict__ feat_out, int* __restrict__ iters_out) {
    __shared__ float c[KM_MAXK][KM_MAXD];
    __shared__ float part[4][KM_MAXK][KM_MAXD];
    __shared__ int cnt_part[4][KM_MAXK];
    __shared__ float red[KM_THREADS / 64];
    __shared__ float shift_sh;
    __shared__ float feat[KM_MAXD];                  // the served pair's feature
    __shared__ float w_row[SP_MAXL];                 // its caption's row of W_sth
    __shared__ int pick_sh;
    extern __shared__ unsigned char choice[];        // [N]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int task = group_task[blockIdx.x];
    if (task < 0 || task >= n_tasks) return;         // unused slot (or a table no host packer writes)
    const int live = min(max(*live_p, 0), P);
    const long long S = (long long)HW + L;
    const float* X = banks + (long long)task * bank_stride;
    float* cg = centers_all + (long long)task * centers_stride;
    for (int i = tid; i < K * D; i += KM_THREADS) c[i / D][i % D] = cg[i];
    __syncthreads();
    for (int p = 0; p < live; ++p) {
        const int cap = pair_caption[p];
        if (cap < 0 || cap >= T) {                   // never an index: the pair is skipped (every live workgroup reports the same p + 1)
            if (tid == 0) atomicMax(status, p + 1);
            continue;
        }
        if (cap_task[cap] != task) continue;
        const bf16_t* text = memory + ((long long)p * S + HW) * D;
        for (int l = tid; l < L; l += KM_THREADS) w_row[l] = W_sth[(long long)cap * L + l];
        __syncthreads();
        if (tid < D) {
#pragma clang fp contract(off)
            float acc = 0.f;
            for (int l = 0; l < L; ++l) {
                const float prod = w_row[l] * bf2f(text[(long long)l * D + tid]);
                acc = acc + prod;
            }
            feat[tid] = acc;
            if (feat_out) feat_out[(long long)p * D + tid] = acc;
        }
        __syncthreads();
        const int it = lloyd_iterations(X, N, D, K, tol, max_iter, c, part, cnt_part, red, &shift_sh, choice);
        for (int i = tid; i < K * D; i += KM_THREADS) cg[i] = c[i / D][i % D];
        if (wave == 0) {
            const int best = nearest_centre(feat, c, D, K, lane);
            if (lane == 0) {
                pick_sh = best;
                if (pick_out) pick_out[p] = best;
                if (iters_out) iters_out[p] = it;
            }
        }
        __syncthreads();
        const int best = pick_sh;
        bf16_t* text_mod = memory_mod + ((long long)p * S + HW) * D;
        for (int i = tid; i < L * D; i += KM_THREADS) {
            const int l = i / D, d = i - l * D;
            if (sub_sth[(long long)cap * L + l]) text_mod[i] = f2bf(c[best][d]);
        }
        __syncthreads();                             // c[], feat[], w_row[] and pick_sh are free for the next pair
    }
}

// ---- FIFO update of the memory banks (mdetr.py:85-97) with its bookkeeping (mdetr.py:90-92), decided on the device ---------------------------------
// One workgroup per group slot; a group is all images of one task, so the workgroup owns that task's bank and its two counters for the launch.
constexpr int FIFO_THREADS = 1024, FIFO_U = 4;

// a[i] = a[i + shift] for i in [0, count), shift > 0: an overlapping move made safe by construction.  Chunks of FIFO_THREADS * FIFO_U elements in
// ascending order; every load of a chunk is in registers before the barrier, its stores come after, and a later chunk only reads elements that no
// earlier chunk has written (stores end below base + chunk, later loads start at base + chunk + shift).
template <typename V>
__device__ __forceinline__ void fifo_shift(V* a, long long shift, long long count, int tid) {
    for (long long base = 0; base < count; base += (long long)FIFO_THREADS * FIFO_U) {
        V v[FIFO_U];
#pragma unroll
        for (int u = 0; u < FIFO_U; ++u) {
            const long long i = base + (long long)u * FIFO_THREADS + tid;
            if (i < count) v[u] = a[i + shift];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < FIFO_U; ++u) {
            const long long i = base + (long long)u * FIFO_THREADS + tid;
            if (i < count) a[i] = v[u];
        }
    }
}

__global__ __launch_bounds__(FIFO_THREADS) void bank_fifo_kernel(float* banks, long long bank_stride, float* update_count, float* full_label,
                                                                 const int* __restrict__ group_task, const int* __restrict__ group_off,
                                                                 const int* __restrict__ members, const float* __restrict__ rows, int T, int B, int N,
                                                                 int D, int fifo_when_full, int vec4, int* __restrict__ lsap_rows) {
    const int tid = threadIdx.x, g = blockIdx.x;
    const int off0 = group_off[g], n = group_off[g + 1] - off0, task = group_task[g];
    if (n <= 0 || n > N || off0 < 0 || off0 + n > B || task < 0 || task >= T) {      // unused slot (or a table no host packer writes): nothing moves
        if (tid == 0) lsap_rows[g] = 0;
        return;
    }
    const float label = full_label[task], count = update_count[task];                // read once; written by one lane after the last barrier
    const bool filling = label == 0.f;
    if (!filling && !fifo_when_full) {                                               // nearest replacement: the LSAP launch behind this one takes the group
        if (tid == 0) lsap_rows[g] = n;
        return;
    }
    float* bank = banks + (long long)task * bank_stride;
    const long long keep = (long long)(N - n) * D, shift = (long long)n * D;
    if (vec4) fifo_shift(reinterpret_cast<float4*>(bank), shift / 4, keep / 4, tid);
    else fifo_shift(bank, shift, keep, tid);
    __syncthreads();                                                                 // every old row has been read: the tail may be overwritten
    for (long long i = tid; i < shift; i += FIFO_THREADS) {
        const int j = (int)(i / D), m = members[off0 + j];
        if (m >= 0 && m < B) bank[keep + i] = rows[(long long)m * D + (i - (long long)j * D)];
    }
    if (tid == 0) {
        lsap_rows[g] = 0;
        if (filling) {                                                               // mdetr.py:90-92: the label looks at the count BEFORE the add
            if (count > (float)N) full_label[task] = 1.f;
            update_count[task] = count + (float)n;
        }
    }
}

// dst[dst_row[i]] = src[src_row[i]] for the rows i with dst_row[i] >= 0 and src_row[i] >= 0 (rows of `d` floats; distinct live destinations).
// The memory-bank replacement of the distillation step under hipGraph replay: which slots are live is decided on the device (an LSAP pair table of
// fixed capacity, its status word), so the write must skip the dead ones instead of sending them to a scratch row the bank does not have.
__global__ __launch_bounds__(256) void scatter_rows_kernel(const float* __restrict__ src, const long long* __restrict__ src_row, float* __restrict__ dst,
                                                            const long long* __restrict__ dst_row, int m, int d) {
    const int i = blockIdx.x;
    const long long sr = src_row[i], dr = dst_row[i];
    if (i >= m || sr < 0 || dr < 0) return;
    for (int e = threadIdx.x; e < d; e += 256) dst[dr * d + e] = src[sr * d + e];
}

}  // namespace toist

using namespace toist;

extern "C" int toist_kmeans(const float* banks, int64_t bank_stride, float* centers, int64_t centers_stride, const int32_t* group_task,
                            const int32_t* group_off, const int32_t* members, int n_groups, const float* features, int N, int D, int K, float tol,
                            int max_iter, int32_t* pick, float* chosen_center, int32_t* iters, void* stream) {
    TOIST_REQUIRE(banks && centers && group_task && group_off && members && features && pick && chosen_center && n_groups > 0, "toist_kmeans: bad args");
    TOIST_REQUIRE(N > 0 && N <= 32768 && D > 0 && D <= KM_MAXD && D > 0 && K > 0 && K <= KM_MAXK && K * D <= KM_THREADS && max_iter > 0 && tol >= 0.f,
                  "toist_kmeans: N <= 32768, D <= %d, K <= %d, K * D <= %d (N=%d D=%d K=%d)", KM_MAXD, KM_MAXK, KM_THREADS, N, D, K);
    hipLaunchKernelGGL(kmeans_kernel, dim3(n_groups), dim3(KM_THREADS), (size_t)((N + 15) & ~15), (hipStream_t)stream, banks, (long long)bank_stride, centers,
                       (long long)centers_stride, group_task, group_off, members, features, N, D, K, tol, max_iter, pick, chosen_center, iters);
    return check_launch("toist_kmeans");
}

extern "C" int toist_scatter_rows_f32(const float* src, const int64_t* src_row, float* dst, const int64_t* dst_row, int m, int d, void* stream) {
    using namespace toist;
    TOIST_REQUIRE(src && src_row && dst && dst_row && m > 0 && d > 0, "toist_scatter_rows_f32: bad arguments");
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(m), dim3(256), 0, (hipStream_t)stream, src, (const long long*)src_row, dst, (const long long*)dst_row, m, d);
    return check_launch("toist_scatter_rows_f32");
}

extern "C" int toist_kmeans_init(const float* banks, int64_t bank_stride, float* centers, int64_t centers_stride, const int32_t* group_task,
                                 const int32_t* group_off, const int32_t* members, int n_groups, const float* features, int N, int D, int K, float tol,
                                 int max_iter, int32_t* pick, float* chosen_center, int32_t* iters, const float* full_label, const int32_t* init_rows,
                                 int32_t* status, void* stream) {
    TOIST_REQUIRE(banks && centers && group_task && group_off && members && features && pick && chosen_center && full_label && init_rows && status &&
                      n_groups > 0, "toist_kmeans_init: bad args");
    TOIST_REQUIRE(N > 0 && N <= 32768 && D > 0 && D <= KM_MAXD && K > 0 && K <= KM_MAXK && K * D <= KM_THREADS && max_iter > 0 && tol >= 0.f,
                  "toist_kmeans_init: N <= 32768, D <= %d, K <= %d, K * D <= %d (N=%d D=%d K=%d)", KM_MAXD, KM_MAXK, KM_THREADS, N, D, K);
    hipLaunchKernelGGL(kmeans_init_kernel, dim3(n_groups), dim3(KM_THREADS), (size_t)((N + 15) & ~15), (hipStream_t)stream, banks, (long long)bank_stride,
                       centers, (long long)centers_stride, group_task, group_off, members, features, N, D, K, tol, max_iter, pick, chosen_center, iters,
                       full_label, init_rows, status);
    return check_launch("toist_kmeans_init");
}

extern "C" int toist_bank_fifo(float* banks, int64_t bank_stride, float* update_count, float* full_label, const int32_t* group_task,
                               const int32_t* group_off, const int32_t* members, int n_groups, const float* rows, int T, int B, int N, int D,
                               int fifo_when_full, int32_t* lsap_rows, void* stream) {
    TOIST_REQUIRE(banks && update_count && full_label && group_task && group_off && members && rows && lsap_rows, "toist_bank_fifo: bad args");
    TOIST_REQUIRE(n_groups > 0 && T > 0 && B > 0 && N > 0 && D > 0 && n_groups <= B && B <= N && bank_stride >= (int64_t)N * D,
                  "toist_bank_fifo: 0 < n_groups <= B <= N, bank_stride >= N * D (n_groups=%d B=%d N=%d D=%d)", n_groups, B, N, D);
    const int vec4 = D % 4 == 0 && bank_stride % 4 == 0 && (uintptr_t)banks % 16 == 0;
    hipLaunchKernelGGL(bank_fifo_kernel, dim3(n_groups), dim3(FIFO_THREADS), 0, (hipStream_t)stream, banks, (long long)bank_stride, update_count, full_label,
                       group_task, group_off, members, rows, T, B, N, D, fifo_when_full, vec4, lsap_rows);
    return check_launch("toist_bank_fifo");
}

extern "C" int toist_sweep_prototypes(const void* memory, void* memory_mod, const int32_t* pair_caption, const int32_t* live, const float* W_sth,
                                      const uint8_t* sub_sth, const int32_t* cap_task, const int32_t* group_task, const float* banks,
                                      int64_t bank_stride, float* centers, int64_t centers_stride, int P, int HW, int L, int T, int n_tasks, int N, int D,
                                      int K, float tol, int max_iter, int32_t* status, int32_t* pick, float* features, int32_t* iters, void* stream) {
    TOIST_REQUIRE(memory && memory_mod && memory != memory_mod && pair_caption && live && W_sth && sub_sth && cap_task && group_task && banks && centers &&
                      status, "toist_sweep_prototypes: bad args");
    TOIST_REQUIRE(P > 0 && HW >= 0 && L > 0 && L <= SP_MAXL && T > 0 && n_tasks > 0 && bank_stride >= (int64_t)N * D && centers_stride >= (int64_t)K * D,
                  "toist_sweep_prototypes: P, T, n_tasks > 0, 0 < L <= %d, strides that hold a bank and its centres (P=%d L=%d T=%d tasks=%d)", SP_MAXL, P,
                  L, T, n_tasks);
    TOIST_REQUIRE(N > 0 && N <= 32768 && D > 0 && D <= KM_MAXD && K > 0 && K <= KM_MAXK && K * D <= KM_THREADS && max_iter > 0 && tol >= 0.f,
                  "toist_sweep_prototypes: N <= 32768, D <= %d, K <= %d, K * D <= %d (N=%d D=%d K=%d)", KM_MAXD, KM_MAXK, KM_THREADS, N, D, K);
    hipLaunchKernelGGL(sweep_prototypes_kernel, dim3(T), dim3(KM_THREADS), (size_t)((N + 15) & ~15), (hipStream_t)stream, (const bf16_t*)memory,
                       (bf16_t*)memory_mod, pair_caption, live, W_sth, sub_sth, cap_task, group_task, banks, (long long)bank_stride, centers,
                       (long long)centers_stride, P, HW, L, T, n_tasks, N, D, K, tol, max_iter, status, pick, features, iters);
    return check_launch("toist_sweep_prototypes");
}
