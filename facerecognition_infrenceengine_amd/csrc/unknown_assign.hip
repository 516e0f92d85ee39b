// Unknown-person clustering for a whole batch of faces in ONE launch: the batch form of
// /root/reference/peopleCount.py:441-449 (first cluster with dot(avg, e) >= thr, else a new cluster) plus
// UnknownPerson.update (:68-75: push into a `depth`-deep deque, detection_count += 1, avg = np.mean(deque)).
//
// The rows depend on each other (row f may hit the cluster row f-1 created or moved), so the batch is walked in
// order by ONE workgroup of 16 waves: no other workgroup ever has to see a write of this launch.  Everything the
// kernel rewrites (avg, hist, the counters) is read through vector loads only, with a workgroup barrier between a
// write and the next row's reads; nothing mutable is `const __restrict__`.
//
// state (int32): [FR_UNKNOWN_N] live clusters, [FR_UNKNOWN_OVERFLOW] rows refused at capacity (sticky), then per
// cluster c at FR_UNKNOWN_HEADER + 3 c: ring length, ring head (the slot the next push writes), detection_count.
// hist[c][slot][512]: the ring fills from slot 0; once full the head is also the oldest row.
#include <climits>
#include "match_scan.h"

#define UA_WAVES 16
#define UA_PER_WAVE 4                           // clusters a wave scores per round: their row loads are in flight together
#define UA_ROUND (UA_WAVES * UA_PER_WAVE)

// a counter this launch may have rewritten: an atomic load never takes the scalar path
__device__ __forceinline__ int ua_counter(int32_t* p) {
    return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}

__global__ __launch_bounds__(UA_WAVES * 64) void unknown_assign_batch(const float* E, const int32_t* take, int F, float thr,
                                                                      float* avg, float* hist, int32_t* state,
                                                                      int capacity, int depth, int32_t* out_cluster,
                                                                      int32_t* out_new, int32_t* out_count) {
    __shared__ int first_hit[2][UA_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // n and the overflow count live in registers for the launch (every thread steps them alike) and go back at the end
    int n = ua_counter(state + FR_UNKNOWN_N), overflow = ua_counter(state + FR_UNKNOWN_OVERFLOW);
    n = n < 0 ? 0 : (n > capacity ? capacity : n);          // a state block that was never zeroed reads no row out of bounds
    unsigned phase = 0;                        // rounds so far: round r reports through first_hit[r & 1]
    for (int f = 0; f < F; ++f) {
        if (take && __builtin_amdgcn_readfirstlane(take[f]) == 0) {
            if (tid == 0) { out_cluster[f] = -1; out_new[f] = 0; out_count[f] = 0; }
            continue;
        }
        const float* e = E + (int64_t)f * GD;
        float qv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) qv[k] = e[lane * 8 + k];
        const float ecol = tid < GD ? e[tid] : 0.f;          // thread t < 512 owns column t of the ring and the mean
        // ---- scan: clusters in index order, UA_ROUND per round; the first round with a passing cluster ends it
        int hit = INT_MAX;
        for (int base = 0; base < n; base += UA_ROUND) {
            float4 g0[UA_PER_WAVE], g1[UA_PER_WAVE];
#pragma unroll
            for (int u = 0; u < UA_PER_WAVE; ++u) {
                const int c = base + wave * UA_PER_WAVE + u;
                const float4* g = reinterpret_cast<const float4*>(avg + (int64_t)(c < n ? c : n - 1) * GD + lane * 8);
                g0[u] = g[0]; g1[u] = g[1];
            }
            int mine = INT_MAX;
#pragma unroll
            for (int u = UA_PER_WAVE - 1; u >= 0; --u) {     // descending: the lowest passing index is kept
                const int c = base + wave * UA_PER_WAVE + u;
                const float s = row_dot_wave8(qv, g0[u], g1[u]);
                if (c < n && s >= thr) mine = c;
            }
            if (lane == 0) first_hit[phase & 1][wave] = mine;
            __syncthreads();
            int m = INT_MAX;
#pragma unroll
            for (int w = 0; w < UA_WAVES; ++w) m = min(m, first_hit[phase & 1][w]);
            ++phase;                                         // the other buffer next: a wave that runs ahead writes there
            m = __builtin_amdgcn_readfirstlane(m);
            if (m != INT_MAX) { hit = m; break; }
        }
        // ---- update
        int cluster, is_new = 0, count = 0, ring_len = 0, ring_head = 0;   // ring_*: the cluster's counters after this row
        if (hit != INT_MAX) {
            cluster = hit;
            int32_t* st = state + FR_UNKNOWN_HEADER + 3 * (int64_t)cluster;
            int len = ua_counter(st), head = ua_counter(st + 1);
            count = ua_counter(st + 2) + 1;
            len = len < 1 ? 1 : (len > depth ? depth : len);            // whatever the state block held, the ring's rows
            head = head < 0 || head >= depth ? 0 : head;                 // stay inside hist[cluster]
            const int K = len < depth ? len + 1 : depth;                 // rows in the ring after the push
            const int next = head + 1 == depth ? 0 : head + 1;
            const int oldest = K < depth ? 0 : next;
            if (tid < GD) {
                float* h = hist + (int64_t)cluster * depth * GD + tid;
                h[(int64_t)head * GD] = ecol;
                float s = 0.f;                                           // np.mean(list(deque), axis=0): oldest first
                int r = oldest;
#pragma unroll 4
                for (int j = 0; j < K - 1; ++j) {
                    s += h[(int64_t)r * GD];
                    r = r + 1 == depth ? 0 : r + 1;
                }
                s += ecol;                                               // the newest row is the one just pushed
                avg[(int64_t)cluster * GD + tid] = s / (float)K;
            }
            ring_len = K; ring_head = next;
        } else if (n < capacity) {
            cluster = n; is_new = 1; count = 1;
            if (tid < GD) {
                avg[(int64_t)cluster * GD + tid] = ecol;                 // the first embedding is the mean as is (:66)
                hist[(int64_t)cluster * depth * GD + tid] = ecol;
            }
            ring_len = 1; ring_head = depth == 1 ? 0 : 1;
            ++n;
        } else {
            cluster = -2;                                                // full: nothing changes, the row is counted
            ++overflow;
        }
        if (tid == 0) { out_cluster[f] = cluster; out_new[f] = is_new; out_count[f] = count; }
        if (cluster >= 0) {
            __syncthreads();                                             // avg / ring before the next row reads them
            // The counters go out only now: on a hit every wave has read them above (they give it the ring slot and K),
            // and a store before this barrier could overtake a slower wave's read.  Their next reader is a later row's
            // update, behind at least one scan barrier (n > 0 from here on), which thread 0 enters with this store done.
            if (tid == 0) {
                int32_t* st = state + FR_UNKNOWN_HEADER + 3 * (int64_t)cluster;
                st[0] = ring_len; st[1] = ring_head; st[2] = count;
            }
        }
    }
    if (tid == 0) { state[FR_UNKNOWN_N] = n; state[FR_UNKNOWN_OVERFLOW] = overflow; }
}

extern "C" int fr_unknown_assign_batch_f32(const float* E, const int32_t* take, int F, int D, float thr, float* avg,
                                           float* hist, int32_t* state, int capacity, int depth, int32_t* out_cluster,
                                           int32_t* out_new, int32_t* out_count, fr_stream_t stream) {
    FR_REQUIRE(D == GD, "fr_unknown_assign_batch_f32: D must be %d (got %d)", GD, D);
    FR_REQUIRE(F >= 0, "fr_unknown_assign_batch_f32: negative size");
    if (F == 0) return FR_OK;
    FR_REQUIRE(E && avg && hist && state && out_cluster && out_new && out_count, "fr_unknown_assign_batch_f32: null pointer");
    FR_REQUIRE(capacity > 0 && depth > 0, "fr_unknown_assign_batch_f32: capacity and depth must be positive (got %d, %d)",
               capacity, depth);
    unknown_assign_batch<<<1, UA_WAVES * 64, 0, fr_stream(stream)>>>(E, take, F, thr, avg, hist, state, capacity, depth,
                                                                    out_cluster, out_new, out_count);
    FR_CHECK_LAUNCH("unknown_assign_batch");
    return FR_OK;
}
