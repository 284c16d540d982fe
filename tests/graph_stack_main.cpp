// Stand-alone exercise of the native graphs' workspace allocator (csrc/graph.hpp Stack), built with the host sanitizers by
// tests/test_graph_stack_cpu.py: every block it hands out is written end to end inside a heap buffer of exactly the declared size, so
// a block that leaves the workspace, overlaps a live one or is misaligned ends the program.  Prints "ok <checks>" and exits 0.
#define L4P_GRAPH_STACK_ONLY
#include "graph.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static int checks = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        ++checks;                                                     \
        if (!(cond)) {                                                \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);        \
            return 1;                                                 \
        }                                                             \
    } while (0)

// the allocation pattern of a graph: two long-lived blocks, a scoped pair released by mark, a larger scoped block, one more block
static int pattern(Stack& s, void* out[6]) {
    out[0] = s.take(1000);
    out[1] = s.take(1);
    const size_t m = s.mark();
    out[2] = s.take(4096);
    out[3] = s.take(300);
    s.release(m);
    const size_t m2 = s.mark();
    out[4] = s.take(70000);
    s.release(m2);
    out[5] = s.take(512);
    return 0;
}
static const size_t sizes[6] = {1000, 1, 4096, 300, 70000, 512};

int main() {
    // size query: no memory, one sentinel, the peak is the largest extent ever live
    Stack dry = Stack::sizing();
    void* d[6];
    pattern(dry, d);
    for (int i = 0; i < 6; ++i) CHECK(d[i] == (void*)256);
    CHECK(dry.peak == 1280 + 70000);  // 1000 -> 1024, 1 -> 1280, then the 70000-byte block
    CHECK(dry.off == 1280 + 512);
    const size_t need = dry.bytes_needed();
    CHECK(need == dry.peak + 256);

    // the same pattern over real memory of exactly that size, at every misalignment of the base
    for (size_t skew = 0; skew < 256; skew += 17) {
        char* buf = (char*)malloc(need + skew);
        Stack s = Stack::over(buf + skew, need);
        void* p[6];
        pattern(s, p);
        for (int i = 0; i < 6; ++i) {
            CHECK(p[i] != nullptr);
            CHECK(((uintptr_t)p[i] & 255) == 0);
            CHECK((char*)p[i] >= buf + skew && (char*)p[i] + sizes[i] <= buf + skew + need);
            memset(p[i], 0xA0 + i, sizes[i]);  // (inside the heap block, or the address sanitizer ends the run)
        }
        CHECK(s.peak == dry.peak && s.off == dry.off);
        // blocks live at the same time are disjoint; a block taken after a release reuses the released bytes
        CHECK((char*)p[0] + sizes[0] <= (char*)p[1] && (char*)p[1] + sizes[1] <= (char*)p[2] && (char*)p[2] + sizes[2] <= (char*)p[3]);
        CHECK(p[4] == p[2] && p[5] == p[2]);
        free(buf);
    }

    // a workspace that is too small: null from the block that does not fit on, nothing handed out beyond the cap, and the
    // allocator goes on counting (the caller reports the first refusal and launches nothing)
    {
        const size_t cap = need / 2;
        char* buf = (char*)malloc(cap);
        Stack s = Stack::over(buf, cap);
        void* p[6];
        pattern(s, p);
        CHECK(p[0] && p[1] && p[2] && p[3] && !p[4] && p[5]);
        for (int i = 0; i < 6; ++i)
            if (p[i]) {
                CHECK((char*)p[i] + sizes[i] <= buf + cap);
                memset(p[i], 0x50 + i, sizes[i]);
            }
        CHECK(s.peak == dry.peak);
        free(buf);
    }
    // ... smaller than the padding to the first boundary: everything is refused
    {
        char* buf = (char*)malloc(512);
        char* base = buf + 1;
        const size_t pad = (size_t)(-(uintptr_t)base & 255);
        Stack s = Stack::over(base, pad ? pad - 1 : 0);
        CHECK(s.cap == 0 && s.take(1) == nullptr);
        Stack z = Stack::over(base, pad);
        CHECK(z.cap == 0 && z.take(0) != nullptr && z.take(1) == nullptr);
        free(buf);
    }
    printf("ok %d\n", checks);
    return 0;
}
