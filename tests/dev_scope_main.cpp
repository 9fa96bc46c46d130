// dev_scope_main.cpp -- bb::DevScope (bblean_amd/csrc/bb_common.h) on the CPU, where its failure paths can be reached.
// The few symbols the scope uses are faked at link time: blocks come from malloc, every call is logged, the n-th
// allocation and the synchronisation can be made to fail.  Built and run by tests/test_dev_scope.py with the address and
// undefined-behaviour sanitizers; prints one "PASS <name>" / "FAIL <name>: ..." line per check.
#include "../bblean_amd/csrc/bb_common.h"

#include <cstdlib>
#include <map>
#include <string>
#include <vector>

namespace {
std::vector<std::string> g_log;      // "alloc" "pin" "sync" "free" "hostfree", in call order
std::map<void*, char> g_live;        // block -> 'd'evice / 'p'inned
int g_allocs = 0, g_fail_alloc = 0;  // the g_fail_alloc-th allocation of either kind fails (0: none)
bool g_fail_sync = false;
bool g_crossed = false;              // a block went to the wrong free

hipError_t fake_alloc(void** p, size_t bytes, char kind) {
    g_log.push_back(kind == 'd' ? "alloc" : "pin");
    if (++g_allocs == g_fail_alloc) return hipErrorOutOfMemory;
    *p = std::malloc(bytes);
    g_live[*p] = kind;
    return hipSuccess;
}
void fake_free(void* p, char kind) {
    g_log.push_back(kind == 'd' ? "free" : "hostfree");
    const auto it = g_live.find(p);
    if (it == g_live.end() || it->second != kind) {
        g_crossed = true;
        return;
    }
    g_live.erase(it);
    std::free(p);
}
void reset(int fail_alloc = 0, bool fail_sync = false) {
    g_log.clear();
    g_allocs = 0;
    g_fail_alloc = fail_alloc;
    g_fail_sync = fail_sync;
}
std::string log_text() {
    std::string s;
    for (const std::string& e : g_log) s += (s.empty() ? "" : " ") + e;
    return s;
}
}  // namespace

namespace bb {
thread_local char g_err[512] = "";
hipError_t dev_alloc(void** p, size_t bytes) { return fake_alloc(p, bytes, 'd'); }
void dev_free(void* p) { fake_free(p, 'd'); }
}  // namespace bb
extern "C" {
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return fake_alloc(p, bytes, 'p'); }
hipError_t hipHostFree(void* p) {
    fake_free(p, 'p');
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
    g_log.push_back("sync");
    return g_fail_sync ? hipErrorLaunchFailure : hipSuccess;
}
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake error"; }
}

namespace {
const int kBlocks = 4;
// a call as the library writes them: three device blocks and a pinned one, every byte touched, closed by sync()
int four_blocks(hipStream_t s) {
    bb::DevScope scope(s);
    uint32_t *a = nullptr, *b = nullptr, *c = nullptr;
    uint8_t* pin = nullptr;
    BB_HIP(scope.get(&a, 16));
    BB_HIP(scope.get(&b, 0));  // (the scope never asks for 0 bytes: 4)
    BB_HIP(scope.pinned(&pin, 64));
    BB_HIP(scope.get(&c, 32));
    std::memset(a, 1, 16);
    std::memset(b, 2, 4);
    std::memset(pin, 3, 64);
    std::memset(c, 4, 32);
    return scope.sync();
}

int g_failed = 0;
void check(const char* name, bool ok) {
    if (ok && !g_crossed && g_live.empty()) {
        std::printf("PASS %s\n", name);
        return;
    }
    ++g_failed;
    std::printf("FAIL %s: log [%s], %zu blocks live, crossed %d, last error \"%s\"\n", name, log_text().c_str(), g_live.size(), (int)g_crossed,
                bb::g_err);
    for (auto& kv : g_live) std::free(kv.first);
    g_live.clear();
    g_crossed = false;
}
}  // namespace

int main() {
    const hipStream_t s = nullptr;
    for (int n = 1; n <= kBlocks; ++n) {
        reset(n);
        const int rc = four_blocks(s);
        const std::string name = "alloc_" + std::to_string(n) + "_fails";
        check(name.c_str(), rc == BBH_ERR_HIP && g_allocs == n);
    }
    {
        reset();
        const int rc = four_blocks(s);
        // (the whole call: after its sync() the destructor frees and does not synchronise again; kinds never crossed)
        check("sync_then_frees_only", rc == BBH_OK && log_text() == "alloc alloc pin alloc sync free free hostfree free");
    }
    {
        reset();
        {
            bb::DevScope scope(s);
            int* a = nullptr;
            (void)scope.get(&a, 8);
        }  // (an early return: no sync())
        check("early_return_syncs_before_free", log_text() == "alloc sync free");
    }
    {
        reset();
        int rc = -1;
        {
            bb::DevScope scope(s);
            int *a = nullptr, *b = nullptr;
            (void)scope.get(&a, 8);
            rc = scope.sync();
            (void)scope.pinned(&b, 8);
        }
        check("get_after_sync_syncs_again", rc == BBH_OK && log_text() == "alloc sync pin sync free hostfree");
    }
    {
        reset(0, true);
        {
            bb::DevScope scope(s);
            int *a = nullptr, *b = nullptr;
            (void)scope.get(&a, 8);
            (void)scope.pinned(&b, 8);
        }
        check("failing_sync_in_destructor_still_frees", log_text() == "alloc pin sync free hostfree");
    }
    {
        reset(0, true);
        const int rc = four_blocks(s);
        // (a sync() that failed does not count: the destructor tries once more before the blocks go)
        check("sync_reports_stream_error", rc == BBH_ERR_HIP && std::string(bb::g_err).find("fake error") != std::string::npos &&
                                               log_text() == "alloc alloc pin alloc sync sync free free hostfree free");
    }
    {
        reset();
        { bb::DevScope scope(s); }
        check("empty_scope_calls_nothing", g_log.empty());
    }
    {
        reset();
        int rc = -1;
        {
            bb::DevScope scope(s);
            rc = scope.sync();  // (a call without scratch blocks still ends in its synchronisation)
        }
        check("sync_without_blocks", rc == BBH_OK && log_text() == "sync");
    }
    return g_failed ? 1 : 0;
}
