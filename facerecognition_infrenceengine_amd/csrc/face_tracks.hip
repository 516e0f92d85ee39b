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
// 4. track_fuse (track templates; include/frhip.h fr_track_fuse_f32, DESIGN.md 4.5g, tests/helpers/track_template_ref.py is the
//    definition): behind track_commit, one wave per (frame, detection slot) keeps a ring of the entry's last K unit rows
//    and their unit mean, and hands that mean out as the scan query.  The dot, the mean and the unit row are the pinned forms
//    of match_scan.h / fr_mean_rows_f32, so the wave holds the row in two lane layouts: eight consecutive floats per lane for
//    the dot, 4 + 4 for everything else.  Safe without atomics for the reasons of 3.; the row written this turn is taken
//    from the registers that hold `normed`, never read back.
#include "match_scan.h"

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

constexpr int TF_NONE = 0, TF_STARTED = 1, TF_JOINED = 2, TF_RESTARTED = 3, TF_READ = 4;

// wave (detection slot j, frame f); lane l holds floats 4l .. 4l+3 and 256 + 4l .. 256 + 4l+3 of a row (unit_row_wave4's layout)
__global__ __launch_bounds__(64) void track_fuse(const int32_t* __restrict__ entry, const int32_t* __restrict__ need,
                                                 const int32_t* __restrict__ tid, const int32_t* __restrict__ slot,
                                                 const int32_t* __restrict__ counts, const float* __restrict__ normed, int cap,
                                                 int S, int T, int K, float join_thr, float* tring, int32_t* ttmpl, float* tmean,
                                                 float* __restrict__ query, int32_t* __restrict__ shots,
                                                 int32_t* __restrict__ event) {
    const int j = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
    const int64_t q = (int64_t)f * cap + j;
    const float4v* __restrict__ n_row = reinterpret_cast<const float4v*>(normed + q * TR_DIM);
    const float4v n0 = n_row[lane], n1 = n_row[64 + lane];
    float4v o0 = n0, o1 = n1;                                   // the query: the row itself unless a template answers
    int len = 0, ev = TF_NONE;
    const int s = slot[f];
    const int e = j < min(max(counts[f], 0), cap) ? entry[q] : -1;
    if (s >= 0 && s < S && e >= 0 && e < T) {                   // wave-uniform, as every branch below
        const int64_t row = (int64_t)s * T + e;
        int4v* trow = reinterpret_cast<int4v*>(ttmpl) + row;
        float4v* m_row = reinterpret_cast<float4v*>(tmean + row * TR_DIM);
        int4v tt = *trow;
        const int id = tid[q];
        const bool holds = tt[0] >= 1 && tt[2] == id;
        if (need[q] != 0) {
            bool join = false;
            if (holds) {                                        // c = dot(n, template), lane l on floats 8l .. 8l+7
                const float4v a0 = n_row[2 * lane], a1 = n_row[2 * lane + 1];
                const float4v g0 = m_row[2 * lane], g1 = m_row[2 * lane + 1];
                const float qv[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                const float c = row_dot_wave8(qv, make_float4(g0.x, g0.y, g0.z, g0.w), make_float4(g1.x, g1.y, g1.z, g1.w));
                join = c >= join_thr;                           // false for a NaN
            }
            ev = !holds ? TF_STARTED : (join ? TF_JOINED : TF_RESTARTED);
            // state this rule did not write at this K (len > K, head outside [0, K)) stays inside the ring all the same
            const int pos = join ? (int)((unsigned)tt[1] % (unsigned)K) : 0;
            len = join ? min(tt[0], K - 1) + 1 : 1;
            const int head = (pos + 1) % K;
            float4v* ring = reinterpret_cast<float4v*>(tring + row * K * TR_DIM);
            ring[pos * (TR_DIM / 4) + lane] = n0;
            ring[pos * (TR_DIM / 4) + 64 + lane] = n1;
            if (len > 1) {                                      // the rows oldest first: fr_mean_rows_f32's sum, then the unit row
                const int start = len == K ? head : 0;
                float4v s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
                for (int i = 0; i < len; ++i) {
                    int r = start + i;
                    if (r >= K) r -= K;
                    float4v v0 = n0, v1 = n1;
                    if (r != pos) {                             // never the row this launch wrote
                        v0 = ring[r * (TR_DIM / 4) + lane];
                        v1 = ring[r * (TR_DIM / 4) + 64 + lane];
                    }
                    s0 += v0;
                    s1 += v1;
                }
                s0 /= (float)len;
                s1 /= (float)len;
                float4 u0 = make_float4(s0.x, s0.y, s0.z, s0.w), u1 = make_float4(s1.x, s1.y, s1.z, s1.w);
                unit_row_wave4(u0, u1);
                o0 = float4v{u0.x, u0.y, u0.z, u0.w};
                o1 = float4v{u1.x, u1.y, u1.z, u1.w};
            }                                                   // len == 1: the row's own bits, no arithmetic
            m_row[lane] = o0;
            m_row[64 + lane] = o1;
            if (lane == 0) {
                const int4v out = {len, head, id, 0};
                *trow = out;
            }
        } else if (holds) {
            ev = TF_READ;
            len = tt[0];
            o0 = m_row[lane];
            o1 = m_row[64 + lane];
        }
    }
    float4v* __restrict__ q_row = reinterpret_cast<float4v*>(query + q * TR_DIM);
    q_row[lane] = o0;
    q_row[64 + lane] = o1;
    if (lane == 0) {
        shots[q] = len;
        event[q] = ev;
    }
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

extern "C" int fr_track_fuse_f32(const int32_t* entry, const int32_t* need, const int32_t* tid, const int32_t* slot,
                                 const int32_t* counts, const float* normed, int N, int cap, int S, int T, int K, float join_thr,
                                 float* tring, int32_t* ttmpl, float* tmean, float* query, int32_t* shots, int32_t* event,
                                 fr_stream_t stream) {
    if (const int rc = track_check("fr_track_fuse_f32", N, cap, S, T)) return rc;
    FR_REQUIRE(K >= 1 && K <= 16, "fr_track_fuse_f32: K %d outside 1 .. 16 shots per template", K);
    FR_REQUIRE(join_thr >= -1.0f && join_thr <= 1.0f, "fr_track_fuse_f32: join_thr %g outside [-1, 1]", (double)join_thr);
    if (N == 0) return FR_OK;
    FR_REQUIRE(entry && need && tid && slot && counts && normed && tring && ttmpl && tmean && query && shots && event,
               "fr_track_fuse_f32: null pointer");
    track_fuse<<<dim3((unsigned)cap, (unsigned)N), 64, 0, fr_stream(stream)>>>(entry, need, tid, slot, counts, normed, cap, S, T, K,
                                                                               join_thr, tring, ttmpl, tmean, query, shots, event);
    FR_CHECK_LAUNCH("track_fuse");
    return FR_OK;
}
