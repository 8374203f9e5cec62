// The context's device caches (csrc/host/device_cache.h) against a counting
// device: the host compiler alone, AddressSanitizer and UBSan, no GPU. What no
// GPU run can provoke runs here: every failed allocation and every failed
// copy of every cache kind, the eviction cascade, and the lifetime of the
// uploads' host sources (the device defers its uploads to drain(), which reads
// the sources then).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <set>
#include <vector>

#include "host/device_cache.h"

namespace {

int g_checks = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        g_checks++;                                                       \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

void* const S = reinterpret_cast<void*>(0x10);     // the caller's stream
void* const LAST = reinterpret_cast<void*>(0x20);  // the context's last launch stream
void* const UP = reinterpret_cast<void*>(0x30);    // the upload stream (release everything)

struct Op {
    char kind;  // 'a'lloc, 'u'pload, 'z'ero, 'f'ree
    void* p;
    size_t bytes;
    void* stream;
};

struct FakeDevice {
    std::vector<Op> log;
    std::map<void*, size_t> live;
    int fail_alloc = 0, fail_copy = 0;  // fails the n-th allocation / copy (upload or zero) from now; 0: none
    struct Upload {
        void* dst;
        const void* src;
        size_t bytes;
    };
    std::vector<Upload> pending;

    bool alloc(void** p, size_t bytes, void* s) {
        if (fail_alloc && --fail_alloc == 0) return false;
        *p = std::malloc(bytes ? bytes : 1);
        std::memset(*p, 0xAB, bytes);
        live[*p] = bytes;
        log.push_back({'a', *p, bytes, s});
        return true;
    }
    bool upload(void* dst, const void* src, size_t bytes, void* s) {
        if (fail_copy && --fail_copy == 0) return false;
        CHECK(live.count(dst) && live[dst] == bytes);
        pending.push_back({dst, src, bytes});
        log.push_back({'u', dst, bytes, s});
        return true;
    }
    bool zero(void* dst, size_t bytes, void* s) {
        if (fail_copy && --fail_copy == 0) return false;
        CHECK(live.count(dst) && live[dst] == bytes);
        std::memset(dst, 0, bytes);
        log.push_back({'z', dst, bytes, s});
        return true;
    }
    void free(void* p, void* s) {
        CHECK(live.count(p) == 1);  // no double free, nothing foreign
        for (size_t i = pending.size(); i-- > 0;)
            if (pending[i].dst == p) pending.erase(pending.begin() + (long)i);
        live.erase(p);
        std::free(p);
        log.push_back({'f', p, 0, s});
    }
    // The stream runs: every upload still wanted reads its source now
    void drain() {
        for (const Upload& u : pending) std::memcpy(u.dst, u.src, u.bytes);
        pending.clear();
    }
    std::vector<Op> frees_since(size_t mark) const {
        std::vector<Op> f;
        for (size_t i = mark; i < log.size(); i++)
            if (log[i].kind == 'f') f.push_back(log[i]);
        return f;
    }
};

// ---- the generic cache: two buffers, the first uploaded, the second zeroed
using Pair = sr_cache::DeviceCache<int, int, 2>;

int get(Pair& c, FakeDevice& d, uint64_t& tick, int key, int** out, int* evicted = nullptr) {
    return c.ensure(
        d, tick, key, S, LAST, 24, [&](std::vector<int>& src) { src.assign(5, key); },
        [&](Pair::Entry&) {
            if (evicted) ++*evicted;
        },
        out);
}

void test_generic() {
    FakeDevice d;
    Pair c;
    uint64_t tick = 0;
    int* first[2] = {};
    CHECK(get(c, d, tick, 0, first) == SR_OK);
    CHECK(d.log.size() == 4 && d.log[0].kind == 'a' && d.log[0].bytes == 20 && d.log[1].kind == 'a' &&
          d.log[1].bytes == 24 && d.log[2].kind == 'u' && d.log[3].kind == 'z');
    for (const Op& o : d.log) CHECK(o.stream == S);
    // a hit: no device call, the same pointers
    int* again[2] = {};
    size_t mark = d.log.size();
    CHECK(get(c, d, tick, 0, again) == SR_OK && d.log.size() == mark);
    CHECK(again[0] == first[0] && again[1] == first[1]);
    // 8 entries; key 0 touched in between, so the 9th key evicts key 1: both buffers, once each, on LAST
    int* p[9][2] = {};
    for (int k = 1; k < 8; k++) CHECK(get(c, d, tick, k, p[k]) == SR_OK);
    CHECK(get(c, d, tick, 0, again) == SR_OK);
    CHECK(c.m.size() == 8 && d.live.size() == 16);
    mark = d.log.size();
    int evicted = 0;
    CHECK(get(c, d, tick, 8, p[8], &evicted) == SR_OK && evicted == 1);
    std::vector<Op> f = d.frees_since(mark);
    CHECK(f.size() == 2 && f[0].p == p[1][0] && f[1].p == p[1][1] && f[0].stream == LAST && f[1].stream == LAST);
    CHECK(c.m.size() == 8 && !c.m.count(1) && c.m.count(0) && d.live.size() == 16);
    d.drain();
    for (auto& kv : c.m) {
        for (int i = 0; i < 5; i++) CHECK(static_cast<int*>(kv.second.dev[0])[i] == kv.first);
        for (int i = 0; i < 6; i++) CHECK(static_cast<int*>(kv.second.dev[1])[i] == 0);
    }
    // failures: the first and the second allocation, the upload, the zero
    // at a full cache, so each failed call has evicted first
    for (int site = 0; site < 4; site++) {
        const size_t live = d.live.size();
        CHECK(c.m.size() == 8);
        (site < 2 ? d.fail_alloc : d.fail_copy) = 1 + site % 2;
        mark = d.log.size();
        int* q[2] = {};
        CHECK(get(c, d, tick, 100 + site, q) == (site < 2 ? SR_E_NOMEM : SR_E_HIP));
        // the eviction that made room stays (its two buffers went on LAST), nothing of the key does
        CHECK(!c.m.count(100 + site) && c.m.size() == 7 && d.live.size() == live - 2);
        const std::vector<Op> ff = d.frees_since(mark);
        const size_t own = site == 0 ? 0 : site == 1 ? 1 : 2;  // what the failed call had allocated
        CHECK(ff.size() == 2 + own && ff[0].stream == LAST && ff[1].stream == LAST);
        for (size_t i = 2; i < ff.size(); i++) CHECK(ff[i].stream == S);  // on the stream of the failed call
        CHECK(d.fail_alloc == 0 && d.fail_copy == 0);
        CHECK(get(c, d, tick, 100 + site, q) == SR_OK && c.m.count(100 + site) && d.live.size() == live);
        d.drain();
    }
    c.release_all(d, UP);
    CHECK(d.live.empty() && c.m.empty());
    for (const Op& o : d.frees_since(d.log.size() - 2)) CHECK(o.stream == UP);
}

// ---- the context's four caches
struct Ctx {
    FakeDevice d;
    sr_cache::Caches c;
    const int* kept[2] = {nullptr, nullptr};
    bool kept_gone = false;
    std::vector<std::vector<int>> lists;  // host lists, alive as a caller's would be

    int table(int steps, int revs, const sr_pre::StepEntry** out) {
        return c.table(
            d, {steps, revs}, S, LAST,
            [&](std::vector<sr_pre::StepEntry>& t) { t.assign((size_t)steps % 7 + 4, sr_pre::StepEntry()); }, out);
    }
    int xtab(float u_f, float dphi, const float** out) {
        return c.xtab(d, u_f, dphi, S, LAST, [&](std::vector<float>& t) { t.assign(6, 1.5f); }, out);
    }
    int order(int gx, const int* list, int** out) {
        return c.order(
            d, std::make_tuple(gx, 3, 0, 0, list, 0), (size_t)gx * 3 * sizeof(int), S, LAST,
            [&](std::vector<int>& o) { o.assign((size_t)gx * 3, gx << 8); }, out);
    }
    int block_list(int id, const int** out) {
        lists.push_back({id, id + 1, -1});
        kept_gone = false;
        return c.block_list(d, lists.back().data(), 3, S, LAST, kept, &kept_gone, out);
    }
    size_t entries() const { return c.tables.m.size() + c.xtabs.m.size() + c.orders.m.size() + c.block_lists.m.size(); }
};

void test_table_schedule() {
    // tests/test_gpu_view_extremes.py test_caches_under_change: 15 launches, 12 pairs, the first three come back
    const int sched[15][2] = {{400, 2}, {300, 2}, {200, 1}, {100, 3}, {400, 1}, {250, 2}, {150, 2}, {350, 3},
                              {120, 1}, {500, 2}, {400, 2}, {300, 2}, {200, 1}, {7, 50},  {400, -1}};
    Ctx x;
    size_t uploads = 0;
    for (const auto& s : sched) {
        const sr_pre::StepEntry* t = nullptr;
        CHECK(x.table(s[0], s[1], &t) == SR_OK && t);
    }
    for (const Op& o : x.d.log) uploads += o.kind == 'u';
    CHECK(uploads == 15);  // the three that return were evicted before: every launch is a miss
    const std::set<std::pair<int, int>> want = {{350, 3}, {120, 1}, {500, 2}, {400, 2}, {300, 2}, {200, 1}, {7, 50}, {400, -1}};
    std::set<std::pair<int, int>> have;
    for (auto& kv : x.c.tables.m) have.insert(kv.first);
    CHECK(have == want && x.d.live.size() == 8);
    x.d.drain();
    x.c.release_all(x.d, UP);
    CHECK(x.d.live.empty());
}

void test_xtab_keys() {
    Ctx x;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const float *a = nullptr, *b = nullptr, *z0 = nullptr, *z1 = nullptr;
    CHECK(x.xtab(nan, 0.1f, &a) == SR_OK);
    size_t mark = x.d.log.size();
    CHECK(x.xtab(nan, 0.1f, &b) == SR_OK && a == b && x.d.log.size() == mark);  // a NaN hits on its own bits
    CHECK(x.xtab(-nan, 0.1f, &b) == SR_OK && a != b);                            // another NaN is another key
    CHECK(x.xtab(0.0f, 0.1f, &z0) == SR_OK && x.xtab(-0.0f, 0.1f, &z1) == SR_OK && z0 != z1);
    mark = x.d.log.size();
    CHECK(x.xtab(-0.0f, 0.1f, &b) == SR_OK && b == z1 && x.d.log.size() == mark);
    CHECK(x.c.xtabs.m.size() == 4);
    x.d.drain();
    x.c.xtabs.release_all(x.d, UP);  // drop_xtabs: the other caches stay
    CHECK(x.d.live.empty() && x.c.xtabs.m.empty());
}

// Fails every allocation and every copy of one kind's ensure in turn; `call`
// makes the same ensure each time, `allocs` and `copies` are its device calls
void inject(Ctx& x, const char* what, int allocs, int copies, const std::function<int()>& call) {
    for (int site = 0; site < allocs + copies; site++) {
        const bool in_alloc = site < allocs;
        const size_t live = x.d.live.size(), entries = x.entries(), mark = x.d.log.size();
        (in_alloc ? x.d.fail_alloc : x.d.fail_copy) = in_alloc ? site + 1 : site - allocs + 1;
        const int rc = call();
        std::printf("%s: failure at %s %d: status %d\n", what, in_alloc ? "allocation" : "copy",
                    in_alloc ? site + 1 : site - allocs + 1, rc);
        CHECK(rc == (in_alloc ? SR_E_NOMEM : SR_E_HIP));
        CHECK(x.entries() == entries && x.d.live.size() == live);  // the key absent, nothing leaked
        const std::vector<Op> f = x.d.frees_since(mark);
        CHECK(f.size() == (size_t)(in_alloc ? site : allocs));  // what the call had allocated, no more
        for (const Op& o : f) CHECK(o.stream == S);             // on the stream of the failed call
        CHECK(x.d.fail_alloc == 0 && x.d.fail_copy == 0);
    }
    CHECK(call() == SR_OK);  // the same key then succeeds
    x.d.drain();
}

void test_failures() {
    Ctx x;
    const sr_pre::StepEntry* t = nullptr;
    const float* xt = nullptr;
    int* oc[2] = {};
    const int* bl = nullptr;
    inject(x, "table", 1, 1, [&] { return x.table(400, 2, &t); });
    inject(x, "xtab", 1, 1, [&] { return x.xtab(0.05f, 0.1f, &xt); });
    // the order: its second allocation, and its memset, apart from the first and the upload
    inject(x, "order", 2, 2, [&] { return x.order(5, nullptr, oc); });
    CHECK(oc[0] && oc[1] && oc[0][0] == 5 << 8 && oc[1][0] == 0);
    x.lists.reserve(64);
    inject(x, "block list", 1, 1, [&] { return x.block_list(1, &bl); });
    CHECK(bl && bl[0] == 1 && bl[2] == -1 && !x.kept_gone);
    CHECK(x.entries() == 4 && x.d.live.size() == 5);
    // a failure neither drops nor reorders what is cached
    const sr_pre::StepEntry* t2 = nullptr;
    CHECK(x.table(400, 2, &t2) == SR_OK && t2 == t);
    x.c.release_all(x.d, UP);
    CHECK(x.d.live.empty() && x.entries() == 0);
}

void test_cascade() {
    for (int variant = 0; variant < 4; variant++) {
        // variant bit 0: the retained frame references the list that goes; bit 1: last_order is one of its orders
        Ctx x;
        x.lists.reserve(64);
        const int* dl[9] = {};
        for (int i = 0; i < 8; i++) CHECK(x.block_list(10 * i, &dl[i]) == SR_OK && !x.kept_gone);
        int *a[2], *b[2], *other[2], *none[2];
        CHECK(x.order(4, dl[0], a) == SR_OK && x.order(5, dl[0], b) == SR_OK);  // two orders of list 0
        CHECK(x.order(4, dl[1], other) == SR_OK && x.order(4, nullptr, none) == SR_OK);
        x.c.last_order = variant & 2 ? b[0] : other[0];
        x.c.last_slots = 15;
        if (variant & 1) x.kept[variant >> 1] = dl[0];  // as kept.fr.block_list, or as kept.d_blocks
        else x.kept[0] = dl[1];
        const size_t mark = x.d.log.size();
        CHECK(x.block_list(80, &dl[8]) == SR_OK);  // the 9th list: list 0, the least recently used, goes
        const std::vector<Op> f = x.d.frees_since(mark);
        std::multiset<void*> freed, want = {a[0], a[1], b[0], b[1], const_cast<int*>(dl[0])};
        for (const Op& o : f) {
            CHECK(o.stream == LAST);
            freed.insert(o.p);
        }
        CHECK(freed == want);  // exactly its orders' buffer pairs and the list, once each
        CHECK(x.c.orders.m.size() == 2 && x.c.block_lists.m.size() == 8);
        CHECK(x.kept_gone == ((variant & 1) != 0));
        if (variant & 2) CHECK(x.c.last_order == nullptr && x.c.last_slots == 0);
        else CHECK(x.c.last_order == other[0] && x.c.last_slots == 15);
        // the survivors still hit
        int* again[2];
        const size_t quiet = x.d.log.size();
        CHECK(x.order(4, dl[1], again) == SR_OK && again[0] == other[0] && again[1] == other[1]);
        CHECK(x.order(4, nullptr, again) == SR_OK && again[0] == none[0] && x.d.log.size() == quiet);
        // an order evicted on its own takes last_order with it, and nothing else
        x.c.last_order = none[0];
        int* o9[2];
        for (int g = 20; g < 26; g++) CHECK(x.order(g, nullptr, o9) == SR_OK);  // 8 orders
        CHECK(x.order(4, dl[1], again) == SR_OK && x.c.last_order == none[0]);  // touched: (4, no list) is the oldest
        CHECK(x.order(30, nullptr, o9) == SR_OK && x.c.last_order == nullptr && x.c.orders.m.size() == 8);
        x.d.drain();
        x.c.release_all(x.d, UP);
        CHECK(x.d.live.empty());
    }
}

void test_sources_and_release() {
    // a mixed history with failed calls and evictions, undrained until the end: every upload the
    // stream still owes reads a live source (ASan), and release everything leaves nothing
    Ctx x;
    x.lists.reserve(256);
    const sr_pre::StepEntry* t = nullptr;
    const float* xt = nullptr;
    int* oc[2];
    const int* bl = nullptr;
    for (int i = 0; i < 40; i++) {
        if (i % 7 == 3) x.d.fail_alloc = 1 + i % 2;
        if (i % 11 == 5) x.d.fail_copy = 1 + i % 2;
        (void)x.table(100 + i % 13, i % 3, &t);
        (void)x.xtab(0.01f * (float)(i % 10), 0.1f, &xt);
        const int rc = x.block_list(i % 12, &bl);
        (void)x.order(2 + i % 9, rc == SR_OK && i % 2 ? bl : nullptr, oc);
        x.d.fail_alloc = x.d.fail_copy = 0;
        if (i % 16 == 15) x.d.drain();
    }
    CHECK(x.c.tables.m.size() <= 8 && x.c.xtabs.m.size() <= 8 && x.c.orders.m.size() <= 8 && x.c.block_lists.m.size() <= 8);
    size_t buffers = x.c.tables.m.size() + x.c.xtabs.m.size() + 2 * x.c.orders.m.size() + x.c.block_lists.m.size();
    CHECK(x.d.live.size() == buffers);
    x.d.drain();
    for (auto& kv : x.c.block_lists.m)
        CHECK(std::memcmp(kv.second.dev[0], kv.first.data(), kv.first.size() * sizeof(int)) == 0);
    for (auto& kv : x.c.orders.m) {
        CHECK(static_cast<int*>(kv.second.dev[0])[0] == std::get<0>(kv.first) << 8);
        CHECK(static_cast<int*>(kv.second.dev[1])[0] == 0);
    }
    x.c.release_all(x.d, UP);
    CHECK(x.d.live.empty() && x.entries() == 0 && x.c.last_order == nullptr);
}

}  // namespace

int main() {
    static_assert(sr_cache::kCacheEntries == 8, "the capacity the tests walk past");
    test_generic();
    test_table_schedule();
    test_xtab_keys();
    test_failures();
    test_cascade();
    test_sources_and_release();
    std::printf("ALL OK: %d checks\n", g_checks);
    return 0;
}
