// The buffer grower of the host API (psyne_amd/csrc/tdt_grow.h) over a fake allocator that counts
// its live blocks and can be told to fail its k-th call.  Checked for each capacity rule: no
// allocation when the need is met; a successful growth drops the old block once, before the new
// one is allocated, and records the rule's capacity; a failed allocation or a failed drop leaves
// (nullptr, 0) and the next call allocates again; a retiring drop keeps the old block alive until
// the list is released, and nothing leaks.  Host code only; built with
// -fsanitize=address,undefined and run directly (tests/test_grow.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "../../psyne_amd/csrc/tdt_grow.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

constexpr int kErrAlloc = -9, kErrFree = -10;

struct FakeAllocator {
    std::set<void *> live;
    std::vector<std::string> log;  // "alloc" / "free" / "retire", in call order
    int calls = 0, fail_at = 0;    // the fail_at-th alloc call fails (1-based; 0: none)
    int frees = 0, fail_free_at = 0;
    size_t last_cap = 0;
    int alloc(uint8_t **out, size_t cap) {
        ++calls;
        log.push_back("alloc");
        if (calls == fail_at) return kErrAlloc;  // (*out stays as it was, like a failed hipMalloc)
        *out = static_cast<uint8_t *>(std::malloc(cap ? cap : 1));
        live.insert(*out);
        last_cap = cap;
        return 0;
    }
    int free(void *p) {
        ++frees;
        log.push_back("free");
        if (frees == fail_free_at) return kErrFree;
        CHECK(live.count(p) == 1);  // a double free, or a pointer the allocator never gave
        live.erase(p);
        std::free(p);
        return 0;
    }
    void release_all() {  // (a failed free leaves its block to the test)
        for (void *p : live) std::free(p);
        live.clear();
    }
};

using Rule = size_t (*)(size_t, size_t);

int count(const std::vector<std::string> &log, const char *what) {
    int n = 0;
    for (const auto &s : log) n += s == what;
    return n;
}

void check_rule(const char *name, Rule rule) {
    std::printf("rule %s\n", name);
    // --- need met: nothing happens; growth: old block dropped once, before the allocation
    {
        FakeAllocator A;
        uint8_t *p = nullptr;
        size_t have = 0;
        auto drop = [&](uint8_t *old) { return A.free(old); };
        auto alloc = [&](uint8_t **out, size_t cap) { return A.alloc(out, cap); };
        CHECK(psy::grow(p, have, 0, rule(0, have), drop, alloc) == 0);  // need 0 of an empty buffer
        CHECK(p == nullptr && have == 0 && A.calls == 0);
        const size_t c1 = rule(1000, 0);
        CHECK(c1 >= 1000);
        CHECK(psy::grow(p, have, 1000, c1, drop, alloc) == 0);
        CHECK(p != nullptr && have == c1 && A.calls == 1 && A.frees == 0 && A.last_cap == c1);
        uint8_t *first = p;
        for (size_t need : {size_t(0), size_t(1), size_t(999), size_t(1000), have}) {
            CHECK(psy::grow(p, have, need, rule(need, have), drop, alloc) == 0);
            CHECK(p == first && have == c1 && A.calls == 1 && A.frees == 0);
        }
        const size_t need2 = have + 1, c2 = rule(need2, have);
        CHECK(c2 >= need2);
        A.log.clear();
        CHECK(psy::grow(p, have, need2, c2, drop, alloc) == 0);
        CHECK(p != nullptr && have == c2 && A.last_cap == c2);
        CHECK(A.log.size() == 2 && A.log[0] == "free" && A.log[1] == "alloc");  // once, and before
        CHECK(A.live.size() == 1 && A.live.count(p) == 1);
        p[0] = 1, p[c2 - 1] = 2;  // (the whole capacity is there)
        CHECK(A.free(p) == 0);
        CHECK(A.live.empty());
    }
    // --- failed allocation: (nullptr, 0), the old block dropped once, a need of 1 allocates again
    for (int fail_at : {1, 2}) {
        FakeAllocator A;
        A.fail_at = fail_at;
        uint8_t *p = nullptr;
        size_t have = 0;
        auto drop = [&](uint8_t *old) { return A.free(old); };
        auto alloc = [&](uint8_t **out, size_t cap) { return A.alloc(out, cap); };
        if (fail_at == 2) {  // (a block to lose)
            CHECK(psy::grow(p, have, 64, rule(64, have), drop, alloc) == 0);
            CHECK(p != nullptr && have == rule(64, 0));
        }
        const size_t need = have + 4096;
        CHECK(psy::grow(p, have, need, rule(need, have), drop, alloc) == kErrAlloc);
        CHECK(p == nullptr && have == 0);
        CHECK(A.frees == fail_at - 1 && A.live.empty());
        const int calls = A.calls;
        CHECK(psy::grow(p, have, 1, rule(1, have), drop, alloc) == 0);  // (a stale size would pass need <= have)
        CHECK(A.calls == calls + 1 && p != nullptr && have == rule(1, 0) && have >= 1);
        CHECK(A.frees == fail_at - 1);  // nothing dropped twice
        CHECK(A.free(p) == 0);
        CHECK(A.live.empty());
    }
    // --- failed drop: the error comes back without an allocation, the pair is (nullptr, 0)
    {
        FakeAllocator A;
        A.fail_free_at = 1;
        uint8_t *p = nullptr;
        size_t have = 0;
        auto drop = [&](uint8_t *old) { return A.free(old); };
        auto alloc = [&](uint8_t **out, size_t cap) { return A.alloc(out, cap); };
        CHECK(psy::grow(p, have, 100, rule(100, have), drop, alloc) == 0);
        const size_t need = have + 1;
        CHECK(psy::grow(p, have, need, rule(need, have), drop, alloc) == kErrFree);
        CHECK(p == nullptr && have == 0 && A.calls == 1 && A.frees == 1);
        CHECK(psy::grow(p, have, 1, rule(1, have), drop, alloc) == 0);  // usable again
        CHECK(p != nullptr && have == rule(1, 0) && A.calls == 2 && A.frees == 1);
        A.release_all();
    }
    // --- retiring drop: the old blocks live until the list is released, then nothing is left
    {
        FakeAllocator A;
        std::vector<void *> retired;
        uint8_t *p = nullptr;
        uint32_t have = 0;  // (a site's own size type)
        auto drop = [&](uint8_t *old) {
            A.log.push_back("retire");
            retired.push_back(old);
            return 0;
        };
        auto alloc = [&](uint8_t **out, size_t cap) { return A.alloc(out, cap); };
        std::vector<uint8_t *> seen;
        size_t need = 10;
        for (int round = 0; round < 4; ++round) {
            const size_t cap = rule(need, have);
            CHECK(psy::grow(p, have, need, cap, drop, alloc) == 0);
            CHECK(p != nullptr && have == cap && have >= need);
            for (uint8_t *q : seen) {
                CHECK(A.live.count(q) == 1);  // alive, and still writable
                q[0] = 7;
            }
            seen.push_back(p);
            need = have + 1;
        }
        CHECK(retired.size() == 3 && A.live.size() == 4 && A.frees == 0);
        CHECK(count(A.log, "retire") == 3 && count(A.log, "alloc") == 4);
        for (void *q : retired) CHECK(A.free(q) == 0);  // the owner's release: every retired block once,
        CHECK(A.free(p) == 0);                          // then the current one
        CHECK(A.live.empty());
    }
}

}  // namespace

int main() {
    check_rule("exact", psy::cap_exact);
    check_rule("double", psy::cap_double);
    check_rule("slot", psy::cap_slot);
    // the rules themselves
    CHECK(psy::cap_exact(10, 1000) == 10 && psy::cap_exact(0, 0) == 0);
    CHECK(psy::cap_double(10, 4) == 10 && psy::cap_double(10, 8) == 16 && psy::cap_double(1, 0) == 1);
    const size_t MiB = size_t(1) << 20;
    CHECK(psy::cap_slot(1, 0) == MiB && psy::cap_slot(MiB, 0) == MiB && psy::cap_slot(MiB + 1, MiB) == 2 * MiB);
    CHECK(psy::cap_slot(5 * MiB, 4 * MiB) == 6 * MiB && psy::cap_slot(9 * MiB, 4 * MiB) == 9 * MiB);
    std::printf("grow: %d failures\n", failures);
    return failures ? 1 : 0;
}
