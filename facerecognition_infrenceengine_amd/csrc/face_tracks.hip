// Face tracks: carry a face's embedding from one frame of a camera to the next, so that only new faces go through align and
// the embed net.  In an active frame nearly every face is one the previous frame of that camera showed a few pixels away; the
// embed net is 24 GFLOP per face and the larger part of a batch step.  The identity is never kept: a carried face's held
// embedding goes through the gallery scan of the current call like any other row.
//
// The rule (include/frhip.h fr_track_associate_f32; tests/helpers/track_ref.py is the definition).  State per
// camera slot s < S, T <= 64 entries: tbox f32 [S,T,4], tstate i32 [S,T,4] = (live, since, misses, id), next_id i32 [S],
// bank f32 [S,T,2,512].  Frame i, detections j = 0 .. counts[i] - 1 in the detector's order, one after the other:
//     o[t]   = IoU(detection j, tbox[t]) of every LIVE entry: float32, one rounding per operation, the "+1" form and operand
//              order nms.hip is pinned to (area = (x2 - x1 + 1) * (y2 - y1 + 1), o = inter / ((area_d + area_t) - inter)); a NaN
//              coordinate on either side makes o NaN
//     match  = among live entries not claimed this turn with o[t] >= iou_thr (a NaN never is), the largest o, the lowest t on
//              equal values; the entry is claimed, its tbox becomes the detection's box, misses = 0
//     carry  = matched, since < max_reuse, and no OTHER live entry (claimed or not) has o[t] > 0: need = 0, since += 1;
//              a matched detection that is not carried: need = 1, since = 0
// then every live unclaimed entry: misses += 1, live = 0 when misses > max_misses; then every unmatched detection in j order
// takes the lowest entry that is not live (id = next_id[s]++, since = misses = 0, need = 1), or stays untracked when none is.
//
// 1. track_associate: one wave per frame, lane t holds entry t in registers.  The argmax is a wave max over the candidates'
//    values and a ballot of the lanes that hold it (candidates are >= iou_thr > 0, so the float order is a total order over
//    them); the guard is a ballot of o > 0.  Nothing is read back from memory inside the loop, the state is written once at
//    the end with one 16-byte store per array and lane.
// 2. track_commit: one workgroup per (frame, detection slot), 128 lanes x 16 bytes per 512-float row.
// 3. track_resolve_quality (judging tracks; include/frhip.h fr_track_resolve_quality_i32, DESIGN.md 4.5f,
//    tests/helpers/track_quality_ref.py is the definition): between the quality launch and the one host copy, one thread per
//    detection slot decides embed, carry or reject from (entry, need, tid) of the associate launch and the verdict, and keeps
//    tqual i32 [S,T,4] = (has, age, id, 0): the entry holds a FIT row for the current track iff has == 1 and id == tstate.id.
//    Safe without atomics or ordering for two reasons: each (slot, entry) is claimed by at most one detection per turn (the
//    associate launch claims an entry once), and a call never names a slot twice (FaceTracks refuses repeats) - so no two
//    threads touch one tqual / tstate row.  Plain vector loads and stores, no LDS, no synchronisation.
#include "common.h"

namespace {

constexpr int TR_DIM = 512;

struct TrackRule { float iou_thr; int max_reuse, max_misses; };

// np.maximum / np.minimum: a NaN operand gives NaN (fmaxf / fminf would drop it)
__device__ __forceinline__ float max_nan(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
__device__ __forceinline__ float min_nan(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

__device__ __forceinline__ float box_area(const float4 b) { return (b.z - b.x + 1.0f) * (b.w - b.y + 1.0f); }

// IoU of detection d (area ad) and entry box b (area ab), the operand order of the detectors' list kernels
__device__ __forceinline__ float box_iou(const float4 d, float ad, const float4 b, float ab) {
    const float xx1 = max_nan(d.x, b.x), yy1 = max_nan(d.y, b.y);
    const float xx2 = min_nan(d.z, b.z), yy2 = min_nan(d.w, b.w);
    const float w = max_nan(0.0f, xx2 - xx1 + 1.0f), h = max_nan(0.0f, yy2 - yy1 + 1.0f);
    const float inter = w * h;
    return inter / (ad + ab - inter);
}

__global__ __launch_bounds__(64) void track_associate(const float* __restrict__ boxes, const int32_t* __restrict__ counts,
                                                      const int32_t* __restrict__ slot, int cap, int S, int T, float* tbox,
                                                      int32_t* tstate, int32_t* next_id, TrackRule k, int32_t* __restrict__ entry,
                                                      int32_t* __restrict__ need, int32_t* __restrict__ tid) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const int s = slot[f];
    const int n = min(max(counts[f], 0), cap);
    const float4* __restrict__ det = reinterpret_cast<const float4*>(boxes) + (int64_t)f * cap;
    int32_t* __restrict__ e_out = entry + (int64_t)f * cap;
    int32_t* __restrict__ n_out = need + (int64_t)f * cap;
    int32_t* __restrict__ t_out = tid + (int64_t)f * cap;
    if (lane < cap && lane >= n) {                              // the slots behind the frame's faces (cap <= 64: one pass)
        e_out[lane] = -1;
        n_out[lane] = 0;
        t_out[lane] = -1;
    }
    if (s < 0 || s >= S) {                                      // a frame without state (wave-uniform): everything is embedded
        if (lane < n) {
            e_out[lane] = -1;
            n_out[lane] = 1;
            t_out[lane] = -1;
        }
        return;
    }
    const bool mine = lane < T;
    float4* sbox = reinterpret_cast<float4*>(tbox) + (int64_t)s * T;
    int4v* sstate = reinterpret_cast<int4v*>(tstate) + (int64_t)s * T;
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
    int4v st = {0, 0, 0, 0};
    if (mine) {
        box = sbox[lane];
        st = sstate[lane];
    }
    bool live = mine && st[0] != 0, claimed = false;
    int since = st[1], misses = st[2], id = st[3];
    float area = box_area(box);
    unsigned long long unmatched = 0ull;                        // bit j: detection j found no entry (wave-uniform)
    for (int j = 0; j < n; ++j) {
        const float4 d = det[j];
        const float o = live ? box_iou(d, box_area(d), box, area) : 0.0f;
        const bool cand = live && !claimed && o >= k.iou_thr;   // false for a NaN
        float best = cand ? o : 0.0f;                           // candidates are >= iou_thr > 0
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) best = fmaxf(best, __shfl_xor(best, m, 64));
        const unsigned long long top = __ballot(cand && o == best);
        if (top == 0ull) {
            unmatched |= 1ull << j;
            continue;
        }
        const int win = __builtin_ctzll(top);                   // the lowest entry among equal values
        const unsigned long long others = __ballot(live && o > 0.0f) & ~(1ull << win);
        if (lane == win) {
            const bool carry = since < k.max_reuse && others == 0ull;
            box = d;
            area = box_area(d);
            misses = 0;
            claimed = true;
            since = carry ? since + 1 : 0;
            e_out[j] = win;
            n_out[j] = carry ? 0 : 1;
            t_out[j] = id;
        }
    }
    if (live && !claimed) {                                     // retire
        misses += 1;
        if (misses > k.max_misses) live = false;
    }
    unsigned long long free_entries = __ballot(mine && !live);
    int nid = next_id[s];
    while (unmatched) {                                         // new tracks, in j order (wave-uniform loop)
        const int j = __builtin_ctzll(unmatched);
        unmatched &= unmatched - 1ull;
        if (free_entries == 0ull) {                             // table full: untracked
            if (lane == 0) {
                e_out[j] = -1;
                n_out[j] = 1;
                t_out[j] = -1;
            }
            continue;
        }
        const int t = __builtin_ctzll(free_entries);
        free_entries &= free_entries - 1ull;
        if (lane == t) {
            box = det[j];
            live = true;
            since = 0;
            misses = 0;
            id = nid;
            e_out[j] = t;
            n_out[j] = 1;
            t_out[j] = nid;
        }
        nid = (int)((unsigned)nid + 1u);
    }
    if (mine) {
        sbox[lane] = box;
        const int4v out = {live ? 1 : 0, since, misses, id};
        sstate[lane] = out;
    }
    if (lane == 0) next_id[s] = nid;
}

// workgroup (detection slot j, frame f): 128 lanes, one 16-byte move each per row
__global__ __launch_bounds__(128) void track_commit(const int32_t* __restrict__ entry, const int32_t* __restrict__ need,
                                                    const int32_t* __restrict__ slot, const int32_t* __restrict__ counts, int cap,
                                                    int S, int T, float* bank, float* emb, float* normed) {
    const int j = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
    const int s = slot[f];
    if (s < 0 || s >= S || j >= counts[f]) return;              // block-uniform
    const int64_t q = (int64_t)f * cap + j;
    const int e = entry[q];
    if (e < 0 || e >= T) return;
    float4v* row = reinterpret_cast<float4v*>(bank + ((int64_t)s * T + e) * 2 * TR_DIM);
    float4v* e_row = reinterpret_cast<float4v*>(emb + q * TR_DIM);
    float4v* n_row = reinterpret_cast<float4v*>(normed + q * TR_DIM);
    if (need[q] != 0) {                                         // embedded this turn: the bank takes the rows
        row[lane] = e_row[lane];
        row[TR_DIM / 4 + lane] = n_row[lane];
    } else {                                                    // carried: the rows come from the bank
        e_row[lane] = row[lane];
        n_row[lane] = row[TR_DIM / 4 + lane];
    }
}

constexpr int TQ_NONE = 0, TQ_EMBED = 1, TQ_CARRY = 2, TQ_REJECT = 3;

// thread q = frame * cap + detection slot
__global__ __launch_bounds__(256) void track_resolve_quality(const int32_t* __restrict__ entry, const int32_t* __restrict__ need,
                                                             const int32_t* __restrict__ tid,
                                                             const int32_t* __restrict__ verdict, const int32_t* __restrict__ slot,
                                                             const int32_t* __restrict__ counts, int total, int cap, int S, int T,
                                                             int32_t* tstate, int32_t* tqual, int max_age,
                                                             int32_t* __restrict__ action, int32_t* __restrict__ need2,
                                                             int32_t* __restrict__ entry2) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= total) return;
    const int f = q / cap, j = q - f * cap;
    int act = TQ_NONE, e = -1;
    if (j < min(max(counts[f], 0), cap)) {
        const int s = slot[f];
        const bool fit = verdict[q] == 0;
        e = entry[q];
        if (s < 0 || s >= S || e < 0 || e >= T) {                  // A: no state behind this face
            act = fit ? TQ_EMBED : TQ_REJECT;
        } else {                                                    // B
            const int64_t row = (int64_t)s * T + e;
            int4v* qrow = reinterpret_cast<int4v*>(tqual) + row;
            int4v tq = *qrow;
            const int id = tid[q];
            const bool valid = tq[0] == 1 && tq[2] == id;
            const bool young = valid && tq[1] < max_age;
            if (need[q] == 0 && young) {
                act = TQ_CARRY;
                tq[1] += 1;
            } else {
                if (fit) {
                    act = TQ_EMBED;
                    tq[0] = 1, tq[1] = 0, tq[2] = id, tq[3] = 0;
                } else {
                    act = TQ_REJECT;
                    if (young) tq[1] += 1;                          // the row stays for a later carry
                    else tq[0] = 0;
                }
                tstate[row * 4 + 1] = 0;                            // since: the next turn starts a new count
            }
            *qrow = tq;
        }
    }
    action[q] = act;
    need2[q] = act == TQ_EMBED ? 1 : 0;
    entry2[q] = (act == TQ_EMBED || act == TQ_CARRY) ? e : -1;
}

// the checks the entries share
int track_check(const char* who, int N, int cap, int S, int T) {
    FR_REQUIRE(N >= 0 && N <= 65535, "%s: bad size (0 .. 65535 frames)", who);
    FR_REQUIRE(cap >= 1 && cap <= 64, "%s: cap %d outside 1 .. 64 detection slots per frame", who, cap);
    FR_REQUIRE(T >= 1 && T <= 64, "%s: T %d outside 1 .. 64 track entries per slot (one lane each)", who, T);
    FR_REQUIRE(S >= 1, "%s: bad state size (S %d camera slots)", who, S);
    return FR_OK;
}

}  // namespace

extern "C" int fr_track_associate_f32(const float* boxes, const int32_t* counts, const int32_t* slot, int N, int cap, int S, int T,
                                      float* tbox, int32_t* tstate, int32_t* next_id, float iou_thr, int max_reuse, int max_misses,
                                      int32_t* entry, int32_t* need, int32_t* tid, fr_stream_t stream) {
    if (const int rc = track_check("fr_track_associate_f32", N, cap, S, T)) return rc;
    FR_REQUIRE(max_reuse >= 0, "fr_track_associate_f32: max_reuse %d below 0 (0: never carry)", max_reuse);
    FR_REQUIRE(max_misses >= 0, "fr_track_associate_f32: max_misses %d below 0", max_misses);
    FR_REQUIRE(iou_thr > 0.0f && iou_thr <= 1.0f, "fr_track_associate_f32: iou_thr %g outside (0, 1]", (double)iou_thr);
    if (N == 0) return FR_OK;
    FR_REQUIRE(boxes && counts && slot && tbox && tstate && next_id && entry && need && tid,
               "fr_track_associate_f32: null pointer");
    track_associate<<<(unsigned)N, 64, 0, fr_stream(stream)>>>(boxes, counts, slot, cap, S, T, tbox, tstate, next_id,
                                                               TrackRule{iou_thr, max_reuse, max_misses}, entry, need, tid);
    FR_CHECK_LAUNCH("track_associate");
    return FR_OK;
}

extern "C" int fr_track_commit_f32(const int32_t* entry, const int32_t* need, const int32_t* slot, const int32_t* counts, int N,
                                   int cap, int S, int T, float* bank, float* emb, float* normed, fr_stream_t stream) {
    if (const int rc = track_check("fr_track_commit_f32", N, cap, S, T)) return rc;
    if (N == 0) return FR_OK;
    FR_REQUIRE(entry && need && slot && counts && bank && emb && normed, "fr_track_commit_f32: null pointer");
    track_commit<<<dim3((unsigned)cap, (unsigned)N), 128, 0, fr_stream(stream)>>>(entry, need, slot, counts, cap, S, T, bank, emb,
                                                                                  normed);
    FR_CHECK_LAUNCH("track_commit");
    return FR_OK;
}

extern "C" int fr_track_resolve_quality_i32(const int32_t* entry, const int32_t* need, const int32_t* tid, const int32_t* verdict,
                                            const int32_t* slot, const int32_t* counts, int N, int cap, int S, int T,
                                            int32_t* tstate, int32_t* tqual, int max_age, int32_t* action, int32_t* need2,
                                            int32_t* entry2, fr_stream_t stream) {
    if (const int rc = track_check("fr_track_resolve_quality_i32", N, cap, S, T)) return rc;
    FR_REQUIRE(max_age >= 0, "fr_track_resolve_quality_i32: max_age %d below 0 (0: never carry)", max_age);
    if (N == 0) return FR_OK;
    FR_REQUIRE(entry && need && tid && verdict && slot && counts && tstate && tqual && action && need2 && entry2,
               "fr_track_resolve_quality_i32: null pointer");
    const int total = N * cap;                                      // <= 65535 * 64
    track_resolve_quality<<<(unsigned)((total + 255) / 256), 256, 0, fr_stream(stream)>>>(
        entry, need, tid, verdict, slot, counts, total, cap, S, T, tstate, tqual, max_age, action, need2, entry2);
    FR_CHECK_LAUNCH("track_resolve_quality");
    return FR_OK;
}
