// select_many.h -- what the six population-selection calls (ssc_*_many over ssc_select_many_item; replay.hip, smartstart.hip)
// share: the table checks every call makes, and the logical-row view of a ring's KDE data set.
#pragma once

#include <stdio.h>

#include "ssc_host.h"

namespace ssc {

typedef const __attribute__((address_space(4))) ssc_select_many_item *const_select_item;   // uniform reads: scalar loads

static inline bool select_item_empty(const ssc_select_many_item &it) { return it.n_ss == 0 || it.count == 0; }
static inline int64_t select_item_size(const ssc_select_many_item &it) {
    return it.count < it.ring.capacity ? it.count : it.ring.capacity;
}

// the table-level checks, then the per-item checks common to all calls; `who` [72] receives "<fn>: item <i>"
static inline int select_table_check(const char *fn, const ssc_select_many_item *h_items, const ssc_select_many_item *d_items,
                                     int32_t n_items) {
    SSC_REQUIRE(n_items >= 1, "%s: n_items %d < 1", fn, n_items);
    if (n_items > 65535) return set_error(SSC_EUNSUPPORTED, "%s: %d items > 65535 (one grid row each)", fn, n_items);
    SSC_REQUIRE(h_items != nullptr && d_items != nullptr, "%s: NULL item array", fn);
    return SSC_OK;
}

static inline int select_item_check(const char *fn, int i, const ssc_select_many_item &it, char *who) {
    snprintf(who, 72, "%s: item %d", fn, i);
    SSC_REQUIRE(it.n_ss >= 0 && it.n_ss <= 4096, "%s: n_ss %d not in 0..4096", who, it.n_ss);
    SSC_REQUIRE(it.count >= 0, "%s: count %lld < 0", who, (long long)it.count);
    if (select_item_empty(it)) return SSC_OK;
    SSC_REQUIRE(it.ring.capacity > 0 && it.n >= 1, "%s: capacity %lld / n %lld", who, (long long)it.ring.capacity, (long long)it.n);
    SSC_REQUIRE(it.ring.obs_dim >= 1 && it.ring.obs_dim <= SSC_MAX_STATE, "%s: obs_dim %d out of range", who, it.ring.obs_dim);
    SSC_REQUIRE(select_item_size(it) <= 0x7fffffffLL, "%s: ring too large for int32 buffer indices", who);
    return SSC_OK;
}

// Logical row L (0 = oldest state; size = the newest record's s2) of a ring's data set, as get_all_states() orders it.
// head = (count - size) % capacity is the ring row of the oldest record: L < size <= capacity and head < capacity, so the
// physical row needs one conditional subtraction, no division.
struct RingRows {
    const float *s, *last;     // last: s2 of the newest record
    int64_t capacity, head, size, stride;
    int od;
    __device__ __forceinline__ const float *row(int64_t j) const {
        const int64_t L = j * stride;
        if (L >= size) return last;
        int64_t p = head + L;
        if (p >= capacity) p -= capacity;
        return s + p * od;
    }
};

static __device__ __forceinline__ RingRows ring_rows(const_select_item it) {
    RingRows r;
    const int64_t cap = it->ring.capacity, count = it->count;
    r.size = count < cap ? count : cap;
    r.capacity = cap;
    r.head = (count - r.size) % cap;
    r.stride = it->stride;
    r.od = it->ring.obs_dim;
    r.s = it->ring.s;
    r.last = it->ring.s2 + ((count - 1) % cap) * r.od;
    return r;
}

}  // namespace ssc
