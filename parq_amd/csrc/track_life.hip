// A life for the tracks of the device-resident store (tracks.hip; include/parq_hip.h: parq_tracks_note, parq_tracks_retire): a
// second, parallel record per scene slot with the stable id, the hit count and the first / last sighting of every track, and the
// launch that removes the tracks nobody has seen for too long.  The store's layout is tracks.hip's and is not changed: `note` only
// reads it, `retire` moves whole rows of it.  The NumPy statements are tests/track_life_cases.py (note_ref, retire_ref).
//
// Both kernels are ONE wavefront per scene of the call, like their neighbours in tracks.hip: the slots arrive by value in chunks
// (SlotChunk), the capacity is a template parameter (512 / 2048), there are no atomics and no scratch, nothing is allocated.  The
// workgroup is one wave, so __syncthreads() is a compiler / memory ordering point (it waits for the wave's outstanding loads and
// stores), not a hardware barrier between waves.  Every number read from device memory is checked before it indexes anything.
#include "common.hpp"

#include <climits>

namespace parq {

namespace {

constexpr int kLifeCapSmall = 512, kLifeCapLarge = 2048;
constexpr int kLifeHdr = 4;                              // step, known, next_uid, retired

struct LifeSlots {
    int32_t slot[kTrackChunk];
};

__device__ __forceinline__ const int32_t* store_slot(const int32_t* store, int slot, int mt) { return store + (int64_t)slot * (2 + 26 * (int64_t)mt); }
__device__ __forceinline__ int32_t* store_slot(int32_t* store, int slot, int mt) { return store + (int64_t)slot * (2 + 26 * (int64_t)mt); }
__device__ __forceinline__ int32_t* life_slot(int32_t* life, int slot, int mt) { return life + (int64_t)slot * (kLifeHdr + 4 * (int64_t)mt); }

// the conditions of `note` on a slot's numbers: n the store's count, k = known, t0 = step, nu = next_uid
__device__ __forceinline__ bool life_valid(int n, int k, int t0, int nu, int mt) {
    return n >= 0 && n <= mt && k >= 0 && k <= n && t0 >= 0 && t0 < INT_MAX && nu >= 0 && (int64_t)nu + (int64_t)(n - k) <= (int64_t)INT_MAX;
}

// One update noted.  The answers of the queries (step 5) are computed FIRST, from the life as the call found it: a query whose
// track is older than this update (id < k) has that track's uid and its hit count plus one (its own id makes seen[id] true), a
// query whose track was born in this update has uid = next_uid + (id - k) and one hit.  Only then, behind an ordering point, is the
// life written (steps 2 - 4), so no lane reads an element that another lane of this call has written.
template <int CAP>
__global__ __launch_bounds__(kWave) void tracks_note_kernel(LifeSlots slots, int b0, const int32_t* __restrict__ store,
                                                            int32_t* __restrict__ life, int mt, const int32_t* __restrict__ track_id, int Q,
                                                            int32_t* __restrict__ uid_out, int32_t* __restrict__ hits_out) {
    __shared__ unsigned char seen[CAP];
    const int lane = threadIdx.x, b = b0 + blockIdx.x;
    const int slot = slots.slot[blockIdx.x];
    int32_t* L = life_slot(life, slot, mt);
    const int n = store_slot(store, slot, mt)[0], t0 = L[0], k = L[1], nu = L[2];
    const int32_t* ids = track_id + (int64_t)b * Q;
    if (mt > CAP || !life_valid(n, k, t0, nu, mt)) {
        for (int q = lane; q < Q; q += kWave) {
            if (uid_out) uid_out[(int64_t)b * Q + q] = -1;
            if (hits_out) hits_out[(int64_t)b * Q + q] = 0;
        }
        return;
    }
    int32_t* uid = L + kLifeHdr;
    int32_t* hits = uid + mt;
    int32_t* first = hits + mt;
    int32_t* last = first + mt;
    for (int t = lane; t < n; t += kWave) seen[t] = 0;
    __syncthreads();
    for (int q = lane; q < Q; q += kWave) {
        const int id = ids[q];
        int u = (id == -1 || id == -2) ? id : -1, h = 0;
        if (id >= 0 && id < n) {
            seen[id] = 1;                                 // lanes that meet on one element all write 1
            if (id < k) {
                const int old = hits[id];
                u = uid[id];
                h = old < INT_MAX ? old + 1 : INT_MAX;
            } else {
                u = nu + (id - k);
                h = 1;
            }
        }
        if (uid_out) uid_out[(int64_t)b * Q + q] = u;
        if (hits_out) hits_out[(int64_t)b * Q + q] = h;
    }
    __syncthreads();                                      // every read of the old life is done, `seen` is complete
    for (int t = lane; t < n; t += kWave) {
        const bool s = seen[t] != 0;
        if (t < k) {
            if (s) {
                const int old = hits[t];
                hits[t] = old < INT_MAX ? old + 1 : INT_MAX;
                last[t] = t0;
            }
        } else {
            uid[t] = nu + (t - k);
            hits[t] = s ? 1 : 0;
            first[t] = t0;
            last[t] = t0;
        }
    }
    if (lane == 0) {
        L[2] = nu + (n - k);
        L[1] = n;
        L[0] = t0 + 1;
    }
}

// The tracks nobody has seen for too long removed, the others moved up in their order.  Why the move may be done in place:
// the tracks are worked through in ascending chunks of 64.  In a chunk every lane first LOADS all 30 words of its own track (label,
// score, 24 corner words, uid, hits, first, last) into registers; a ballot over the kept lanes, the population count of the lanes
// below and the running base `m` give each kept lane its destination; behind an ordering point the lanes STORE.  A destination is
// base + (kept tracks before this one) <= source, so a store of chunk c lands on a row below (c + 1) * 64: on a row of an earlier
// chunk, already read, or of this chunk, whose loads all precede its stores.  No store can land on a row that a later chunk still
// has to read, and within a chunk the destinations of the kept lanes are distinct.  Rows from the final m on are never written.
template <int CAP>
__global__ __launch_bounds__(kWave) void tracks_retire_kernel(LifeSlots slots, int b0, int32_t* __restrict__ store, int32_t* __restrict__ life,
                                                              int mt, int min_hits, int max_age, int tentative_age,
                                                              int32_t* __restrict__ remap_out) {
    const int lane = threadIdx.x, b = b0 + blockIdx.x;
    const int slot = slots.slot[blockIdx.x];
    int32_t* S = store_slot(store, slot, mt);
    int32_t* L = life_slot(life, slot, mt);
    const int n = S[0], t0 = L[0], k = L[1], nu = L[2];
    int32_t* remap = remap_out ? remap_out + (int64_t)b * mt : nullptr;
    if (mt > CAP || !life_valid(n, k, t0, nu, mt) || k != n) {
        if (remap)
            for (int t = lane; t < mt; t += kWave) remap[t] = -1;
        return;
    }
    int32_t* labels = S + 2;
    int32_t* scores = labels + mt;                       // float32 bits: moved as words
    int32_t* corners = scores + mt;
    int32_t* uid = L + kLifeHdr;
    int32_t* hits = uid + mt;
    int32_t* first = hits + mt;
    int32_t* last = first + mt;
    int m = 0;
#pragma unroll 1
    for (int c0 = 0; c0 < CAP && c0 < n; c0 += kWave) {
        const int t = c0 + lane;
        const bool live = t < n;
        int32_t lab = 0, sc = 0, u = 0, h = 0, f = 0, l = 0, cw[24];
#pragma unroll
        for (int i = 0; i < 24; ++i) cw[i] = 0;
        if (live) {
            lab = labels[t];
            sc = scores[t];
            u = uid[t];
            h = hits[t];
            f = first[t];
            l = last[t];
            const int32_t* src = corners + (int64_t)t * 24;
#pragma unroll
            for (int i = 0; i < 24; ++i) cw[i] = src[i];
        }
        const int64_t age = ((int64_t)t0 - 1) - (int64_t)l;
        const bool confirmed = h >= min_hits;
        const bool drop = confirmed ? (max_age >= 0 && age > (int64_t)max_age) : (tentative_age >= 0 && age > (int64_t)tentative_age);
        const bool keep = live && !drop;
        const unsigned long long votes = __ballot(keep);
        const int dst = m + __popcll(votes & ((1ull << lane) - 1ull));
        __syncthreads();                                  // every load of this chunk has returned before its first store
        if (keep && dst != t) {
            labels[dst] = lab;
            scores[dst] = sc;
            uid[dst] = u;
            hits[dst] = h;
            first[dst] = f;
            last[dst] = l;
            int32_t* out = corners + (int64_t)dst * 24;
#pragma unroll
            for (int i = 0; i < 24; ++i) out[i] = cw[i];
        }
        if (remap && live) remap[t] = keep ? dst : -1;
        m += __popcll(votes);
    }
    if (remap)
        for (int t = n + lane; t < mt; t += kWave) remap[t] = -1;
    if (lane == 0 && m != n) {
        const int64_t gone = (int64_t)L[3] + (int64_t)(n - m);
        S[0] = m;
        L[1] = m;
        L[3] = gone < (int64_t)INT_MAX ? (int32_t)gone : INT_MAX;
    }
}

inline LifeSlots life_slots(const int32_t* slots_host, int b0, int nb) {
    LifeSlots s;
    for (int i = 0; i < kTrackChunk; ++i) s.slot[i] = i < nb ? slots_host[b0 + i] : 0;
    return s;
}

}  // namespace

hipError_t launch_tracks_note(const int32_t* store, int32_t* life, int max_tracks, const int32_t* slots_host, int b0, int nb,
                              const int32_t* track_id, int Q, int32_t* uid_out, int32_t* hits_out, hipStream_t s) {
    if (nb < 1 || nb > kTrackChunk || Q < 1 || Q > kLifeCapLarge || max_tracks < 1 || max_tracks > kLifeCapLarge) return hipErrorInvalidValue;
    const LifeSlots slots = life_slots(slots_host, b0, nb);
    if (max_tracks <= kLifeCapSmall)
        hipLaunchKernelGGL(tracks_note_kernel<kLifeCapSmall>, dim3((unsigned)nb), dim3(kWave), 0, s, slots, b0, store, life, max_tracks, track_id,
                           Q, uid_out, hits_out);
    else
        hipLaunchKernelGGL(tracks_note_kernel<kLifeCapLarge>, dim3((unsigned)nb), dim3(kWave), 0, s, slots, b0, store, life, max_tracks, track_id,
                           Q, uid_out, hits_out);
    return hipGetLastError();
}

hipError_t launch_tracks_retire(int32_t* store, int32_t* life, int max_tracks, const int32_t* slots_host, int b0, int nb, int min_hits,
                                int max_age, int tentative_age, int32_t* remap_out, hipStream_t s) {
    if (nb < 1 || nb > kTrackChunk || max_tracks < 1 || max_tracks > kLifeCapLarge || min_hits < 1) return hipErrorInvalidValue;
    const LifeSlots slots = life_slots(slots_host, b0, nb);
    if (max_tracks <= kLifeCapSmall)
        hipLaunchKernelGGL(tracks_retire_kernel<kLifeCapSmall>, dim3((unsigned)nb), dim3(kWave), 0, s, slots, b0, store, life, max_tracks,
                           min_hits, max_age, tentative_age, remap_out);
    else
        hipLaunchKernelGGL(tracks_retire_kernel<kLifeCapLarge>, dim3((unsigned)nb), dim3(kWave), 0, s, slots, b0, store, life, max_tracks,
                           min_hits, max_age, tentative_age, remap_out);
    return hipGetLastError();
}

}  // namespace parq
