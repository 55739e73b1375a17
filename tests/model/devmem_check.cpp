// devmem_check.cpp -- lz-ani_amd/csrc/lzani_devmem.h on the host alone: DevMem and PinMem under the allocation fault
// (alloc_fault_arm) with every attempt refused, so that the HIP runtime is never called and no GPU is needed.  What is
// checked: a refused alloc / reserve leaves get() == nullptr and capacity() == 0 and returns hipErrorOutOfMemory; move
// construction, move assignment and reset keep that; both kinds of memory count as attempts; the range [first, first +
// count) is exact; disarming stops the refusals (seen from the counter alone: a granted attempt would call the runtime).
// Built and run by tests/test_devmem.py under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "lzani_devmem.h"

using namespace lzani;

static int checks = 0;
#define CHECK(x)                                                                   \
    do {                                                                           \
        ++checks;                                                                  \
        if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } \
    } while (0)

template <class M>
static bool empty(const M& m) { return m.get() == nullptr && m.capacity() == 0 && m.bytes() == 0 && !m; }

static const uint64_t ALL = (uint64_t)1 << 63;

int main()
{
    // ---- every attempt refused: the two kinds, alloc and reserve, sizes 0 and large
    alloc_fault_arm(1, ALL);
    {
        DevMem<int> d;
        PinMem<char> p;
        CHECK(empty(d) && empty(p));
        CHECK(d.alloc(100) == hipErrorOutOfMemory && empty(d));
        CHECK(p.alloc(100) == hipErrorOutOfMemory && empty(p));
        CHECK(d.alloc(0) == hipErrorOutOfMemory && empty(d));                       // (a count of 0 asks for one element: an attempt too)
        CHECK(d.reserve(1) == hipErrorOutOfMemory && empty(d));
        CHECK(d.reserve((size_t)1 << 40) == hipErrorOutOfMemory && empty(d));
        CHECK(p.reserve(7) == hipErrorOutOfMemory && empty(p));
        CHECK(d.reserve(0) == hipSuccess && empty(d));                              // nothing asked for: no attempt, and still empty
        d.reset(); p.reset();
        CHECK(empty(d) && empty(p));
        // moves of a buffer that a refusal emptied
        DevMem<int> e(std::move(d));
        CHECK(empty(e) && empty(d));
        DevMem<int> f;
        CHECK(f.alloc(3) == hipErrorOutOfMemory);
        f = std::move(e);
        CHECK(empty(f) && empty(e));
        f = std::move(f);                                                           // (self-assignment is a no-op)
        CHECK(empty(f));
        DevMem<int> g;
        g = DevMem<int>();                                                          // "dropping a group is assigning a fresh one"
        CHECK(empty(g));
    }
    CHECK(alloc_fault_arm(1, ALL) == 7);                                            // 2 + 1 + 2 + 1 of the block above, and f's; reserve(0) none

    // ---- got() reads a refusal as "not had" (and calls hipGetLastError only: no device is opened by it)
    {
        DevMem<double> d;
        CHECK(!got(d.alloc(5)) && empty(d));
        CHECK(got(hipSuccess));
    }
    CHECK(alloc_fault_arm(0, 0) == 1);

    // ---- disarmed: attempts are counted, none refused.  (Read off the decision itself: a granted attempt would go to the runtime.)
    CHECK(!alloc_refused() && !alloc_refused() && !alloc_refused());
    CHECK(alloc_fault_arm(3, 2) == 3);

    // ---- the range: attempts 3 and 4 from the arming, and only they
    CHECK(!alloc_refused());            // 1
    CHECK(!alloc_refused());            // 2
    {
        DevMem<short> d;
        PinMem<short> p;
        CHECK(d.alloc(9) == hipErrorOutOfMemory && empty(d));                       // 3
        CHECK(p.alloc(9) == hipErrorOutOfMemory && empty(p));                       // 4
    }
    CHECK(!alloc_refused());            // 5
    CHECK(!alloc_refused());            // 6
    CHECK(alloc_fault_arm(2, 1) == 6);
    CHECK(!alloc_refused());
    CHECK(alloc_refused());
    CHECK(!alloc_refused());
    CHECK(alloc_fault_arm(1, ALL) == 3);
    for (int k = 0; k < 1000; ++k) CHECK(alloc_refused());                          // "from k on": no end
    CHECK(alloc_fault_arm(0, ALL) == 1000);                                         // first == 0 disarms whatever the count
    CHECK(!alloc_refused());
    CHECK(alloc_fault_arm(0, 0) == 1);
    CHECK(alloc_fault_arm(0, 0) == 0);
    printf("devmem_check ok %d\n", checks);
    return 0;
}
