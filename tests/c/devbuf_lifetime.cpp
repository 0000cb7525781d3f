// devbuf_lifetime.cpp -- DevBuf<T> (csrc/handle.hpp) over a counting fake of hipMalloc / hipFree: every allocation is freed
// exactly once, whatever sequence of alloc / ensure / reset / move / destruction it went through, and a failed allocation
// leaves the buffer empty.  Host code only: the definitions below take the place of the runtime's in this program, no GPU
// is touched.  Prints one JSON line (tests/test_boundary.py); exit status 1 on the first violated expectation.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

#include "handle.hpp"

thread_local std::string g_err;

namespace {
std::map<void*, size_t> live;         // pointer -> bytes asked for
int mallocs = 0, frees = 0, bad_frees = 0, fail_next = 0;
size_t last_bytes = 0;
}  // namespace

extern "C" hipError_t hipMalloc(void** p, size_t bytes) {
    if (fail_next > 0) { fail_next--; *p = reinterpret_cast<void*>(0xdead); return hipErrorOutOfMemory; }   // (a dangling value to catch)
    *p = malloc(bytes ? bytes : 1);
    live[*p] = bytes; last_bytes = bytes; mallocs++;
    return hipSuccess;
}
extern "C" hipError_t hipFree(void* p) {
    auto it = live.find(p);
    if (it == live.end()) { bad_frees++; return hipErrorInvalidValue; }   // double free, or a pointer never handed out
    live.erase(it); free(p); frees++;
    return hipSuccess;
}

#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

int main() {
    mallocs = frees = bad_frees = 0; live.clear();
    {
        DevBuf<double> a;
        EXPECT(a.get() == nullptr && a.count() == 0 && !a);
        EXPECT(a.alloc(10) == hipSuccess && a.get() && a.count() == 10 && last_bytes == 10 * sizeof(double));
        double* p = a;                                        // implicit T*
        EXPECT(a.alloc(20) == hipSuccess && a.get() == p && a.count() == 10 && mallocs == 1);    // alloc: once
        EXPECT(a.ensure(10) == hipSuccess && a.ensure(3) == hipSuccess && a.get() == p && mallocs == 1 && frees == 0);   // no grow
        EXPECT(a.ensure(11) == hipSuccess && a.count() == 11 && mallocs == 2 && frees == 1 && live.size() == 1);       // grow
        a.reset();
        EXPECT(!a && a.count() == 0 && frees == 2 && live.empty());
        a.reset();                                            // (an empty buffer: nothing to free)
        EXPECT(frees == 2 && bad_frees == 0);
        EXPECT(a.ensure(4) == hipSuccess && a.count() == 4 && mallocs == 3);   // ensure on an empty buffer allocates

        DevBuf<int> z;                                        // a count of 0 allocates one element
        EXPECT(z.alloc(0) == hipSuccess && z.get() && z.count() == 0 && last_bytes == sizeof(int));
        EXPECT(z.ensure(0) == hipSuccess && mallocs == 4);

        DevBuf<double> b(std::move(a));                       // move construction: one owner
        EXPECT(!a && a.count() == 0 && b.get() && b.count() == 4 && mallocs == 4);
        DevBuf<double> c;
        EXPECT(c.alloc(7) == hipSuccess && mallocs == 5);
        c = std::move(b);                                     // move assignment frees what the target held
        EXPECT(!b && c.count() == 4 && frees == 3 && live.size() == 2);
        DevBuf<double>& self = c;
        c = std::move(self);                                  // (self-move keeps it)
        EXPECT(c.get() && c.count() == 4 && frees == 3);

        fail_next = 1;                                        // failure on an empty buffer
        DevBuf<double> f;
        EXPECT(f.alloc(5) == hipErrorOutOfMemory && f.get() == nullptr && f.count() == 0);
        fail_next = 1;                                        // failure while growing: the old memory is gone, nothing dangles
        EXPECT(c.ensure(100) == hipErrorOutOfMemory && c.get() == nullptr && c.count() == 0 && frees == 4);
        EXPECT(c.ensure(100) == hipSuccess && c.count() == 100 && mallocs == 6);
    }   // z, c destroyed; a, b, f are empty
    EXPECT(live.empty() && mallocs == 6 && frees == 6 && bad_frees == 0);
    printf("{\"mallocs\": %d, \"frees\": %d, \"bad_frees\": %d, \"live\": %zu}\n", mallocs, frees, bad_frees, live.size());
    return 0;
}
