// device_cache.h — the device caches of a context (sr_api.cpp): one keyed,
// bounded LRU cache of stream-ordered device buffers, and the context's four
// on top of it with their relations. No HIP header: the device is a policy
//     bool alloc(void** p, size_t bytes, void* stream)
//     bool upload(void* dst, const void* src, size_t bytes, void* stream)
//     bool zero(void* dst, size_t bytes, void* stream)
//     void free(void* p, void* stream)
// (stream-ordered; a stream is an opaque token), so the failure paths no GPU
// run can provoke run on the CPU (tests/cpp/test_device_cache.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <map>
#include <tuple>
#include <utility>
#include <vector>

#include "host/precompute.h"
#include "sr/sr.h"

namespace sr_cache {

// A cache holds at most this many entries; the least recently used goes.
constexpr size_t kCacheEntries = 8;

// Key -> N device buffers: the first uploaded from the entry's host source (a
// vector of T), the others zero-filled. The source lives exactly as long as
// the entry: the upload is stream-ordered and may read it any time until then.
template <class Key, class T, int N>
struct DeviceCache {
    struct Entry {
        void* dev[N] = {};
        std::vector<T> src;
        uint64_t used = 0;  // the LRU clock's reading at the last ensure
    };
    std::map<Key, Entry> m;

    // The entry's buffers freed on `s`, the entry and its source gone
    template <class Dev, class It>
    It drop(Dev& d, It it, void* s) {
        for (void* p : it->second.dev)
            if (p) d.free(p, s);
        return m.erase(it);
    }

    // The buffers of `key` into out[0 .. N - 1]. A hit makes no device call. A
    // miss evicts down to kCacheEntries - 1 entries (evicted(entry), then its
    // buffers freed on `last`: the context's last launch stream, after its
    // in-flight frames), has build(src) fill the source and allocates, then
    // fills, every buffer (the zeroed ones have `zero_bytes`) on the caller's
    // stream `s`, ahead of the launch that reads them. SR_E_NOMEM on a failed
    // allocation, SR_E_HIP on a failed upload or zero: what was allocated is
    // then freed on `s` and nothing of the key stays.
    template <class Dev, class Build, class Evicted, class P>
    int ensure(Dev& d, uint64_t& tick, const Key& key, void* s, void* last, size_t zero_bytes, Build&& build,
               Evicted&& evicted, P** out) {
        auto it = m.find(key);
        if (it == m.end()) {
            while (m.size() >= kCacheEntries) {
                auto victim = m.begin();
                for (auto i = m.begin(); i != m.end(); ++i)
                    if (i->second.used < victim->second.used) victim = i;
                evicted(victim->second);
                drop(d, victim, last);
            }
            it = m.emplace(key, Entry{}).first;
            Entry& e = it->second;
            build(e.src);
            const size_t bytes[2] = {e.src.size() * sizeof(T), zero_bytes};
            int rc = SR_OK;
            for (int i = 0; i < N && rc == SR_OK; i++)
                if (!d.alloc(&e.dev[i], bytes[i != 0], s)) {
                    e.dev[i] = nullptr;
                    rc = SR_E_NOMEM;
                }
            for (int i = 0; i < N && rc == SR_OK; i++) {
                const bool ok = i ? d.zero(e.dev[i], zero_bytes, s) : d.upload(e.dev[0], e.src.data(), bytes[0], s);
                if (!ok) rc = SR_E_HIP;
            }
            if (rc != SR_OK) {
                drop(d, it, s);
                return rc;
            }
        }
        it->second.used = ++tick;
        for (int i = 0; i < N; i++) out[i] = static_cast<P*>(it->second.dev[i]);
        return SR_OK;
    }

    // Every entry's buffers freed on `s`, the cache empty
    template <class Dev>
    void release_all(Dev&& d, void* s) {
        for (auto it = m.begin(); it != m.end();) it = drop(d, it, s);
    }
};

// The four caches of a context on one LRU clock, and what hangs on them: the
// launch codes of the context's last frame (last_order, an order's first
// buffer) go with that order, and an evicted block list takes the orders keyed
// by it and the retained frame with it. Each ensure takes the caller's stream
// `s` and the context's last launch stream `last` as DeviceCache::ensure does.
struct Caches {
    // (max_steps, max_revolutions) -> the step table
    using TableKey = std::pair<int, int>;
    DeviceCache<TableKey, sr_pre::StepEntry, 1> tables;
    // the bits of (u_f, max_dphi) -> the sequence's exclusion table. Bits: a
    // NaN hits on its own pattern, -0.0 and 0.0 are two keys
    DeviceCache<std::pair<uint32_t, uint32_t>, float, 1> xtabs;
    // (gx, gy, split_tiles, split_log2, block list, projection) -> the launch
    // order (uploaded) and the tiles' costs (zeroed). The list is its device
    // copy: its tiles have their own costs, and so have a projection's frames
    using OrderKey = std::tuple<int, int, int, int, const int*, int>;
    DeviceCache<OrderKey, int, 2> orders;
    // a block list's content -> its device copy
    DeviceCache<std::vector<int>, int, 1> block_lists;
    uint64_t tick = 0;
    const int* last_order = nullptr;
    size_t last_slots = 0;

    template <class Dev, class Build, class P>
    int table(Dev&& d, TableKey key, void* s, void* last, Build&& build, P** dev) {
        return tables.ensure(d, tick, key, s, last, 0, build, [](auto&) {}, dev);
    }

    template <class Dev, class Build, class P>
    int xtab(Dev&& d, float u_f, float max_dphi, void* s, void* last, Build&& build, P** dev) {
        std::pair<uint32_t, uint32_t> key;
        memcpy(&key.first, &u_f, sizeof u_f);
        memcpy(&key.second, &max_dphi, sizeof max_dphi);
        return xtabs.ensure(d, tick, key, s, last, 0, build, [](auto&) {}, dev);
    }

    void forget_order(const void* order) {
        if (last_order == order) {
            last_order = nullptr;
            last_slots = 0;
        }
    }

    // dev[0]: the launch codes build(src) fills, dev[1]: `cost_bytes` of costs
    template <class Dev, class Build>
    int order(Dev&& d, const OrderKey& key, size_t cost_bytes, void* s, void* last, Build&& build, int** dev) {
        return orders.ensure(d, tick, key, s, last, cost_bytes, build, [&](auto& o) { forget_order(o.dev[0]); }, dev);
    }

    // *kept_gone is set when a list goes that the retained frame references
    // (kept[0], kept[1]: its lists' device copies, or null)
    template <class Dev>
    int block_list(Dev&& d, const int* blocks, int n, void* s, void* last, const int* const kept[2], bool* kept_gone,
                   const int** dev) {
        const std::vector<int> key(blocks, blocks + n);
        return block_lists.ensure(
            d, tick, key, s, last, 0, [&](std::vector<int>& src) { src = key; },
            [&](auto& b) {
                for (auto o = orders.m.begin(); o != orders.m.end();) {
                    if (std::get<4>(o->first) == b.dev[0]) {
                        forget_order(o->second.dev[0]);
                        o = orders.drop(d, o, last);
                    } else {
                        ++o;
                    }
                }
                if (b.dev[0] == kept[0] || b.dev[0] == kept[1]) *kept_gone = true;
            },
            dev);
    }

    template <class Dev>
    void release_all(Dev&& d, void* s) {
        tables.release_all(d, s);
        xtabs.release_all(d, s);
        orders.release_all(d, s);
        block_lists.release_all(d, s);
        forget_order(last_order);
    }
};

}  // namespace sr_cache
