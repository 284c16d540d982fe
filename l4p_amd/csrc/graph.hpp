// What the native graphs (api.hip: encoder, api_dpt.hip: DPT decoder, api_trackwin.hip: tracker window) share: the workspace
// allocator, the weight lookup, the launch guard and the dense GEMM descriptor.  Nothing else in the library has a bump allocator,
// a weight lookup or a launch guard.
#pragma once
#include <stddef.h>
#include <stdint.h>

// Bump allocator over a caller-provided workspace: 256-byte steps, LIFO release (m = mark(); ...; release(m)) and a high-water
// mark.  A size query runs the same graph on a dry allocator (no memory behind it: every take() returns the same non-null
// sentinel) and reads the peak.  A workspace that is too small is refused (take() returns null), never overrun.
// (Plain C++: tests/graph_stack_main.cpp compiles this struct alone, L4P_GRAPH_STACK_ONLY, under the host sanitizers.)
struct Stack {
    char* base;
    size_t off, cap, peak;
    bool dry;
    static Stack sizing() { return Stack{nullptr, 0, 0, 0, true}; }
    static Stack over(void* workspace, size_t bytes) {
        const size_t pad = (size_t)(-(uintptr_t)workspace & 255);  // to the next 256-byte boundary
        return Stack{(char*)workspace + pad, 0, bytes > pad ? bytes - pad : 0, 0, false};
    }
    void* take(size_t bytes) {
        const size_t a = (off + 255) & ~(size_t)255;
        off = a + bytes;
        if (off > peak) peak = off;
        return dry ? (void*)256 : (off <= cap ? base + a : nullptr);
    }
    size_t mark() const { return off; }
    void release(size_t m) { off = m; }
    size_t bytes_needed() const { return peak + 256; }  // (the slack covers the alignment of any base)
};

#ifndef L4P_GRAPH_STACK_ONLY
#include <string.h>

#include <string>

#include "engine.hpp"

// the fields every dense product sets: out = A[M][K] (row stride lda) @ W[N][K]^T (row stride ldw); the caller adds what differs
// (bias, activation, residuals, outputs, row maps, conv geometry, another epilogue)
inline GemmParams dense(const void* A, long long M, int K, long long lda, const void* W, long long ldw, int N) {
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = A, p.lda = lda, p.W = W, p.ldw = ldw, p.M = (int)M, p.N = N, p.K = K;
    p.epi = EPI_DENSE;
    return p;
}

// State of one run of a graph.  The first error sticks in rc: allocation and weight lookup report it once, and launch() starts
// nothing after it, so a graph is written straight through and returns rc at its end.
struct Graph {
    const l4p_engine* e;
    hipStream_t st = nullptr;
    int dt, es;
    Stack ws = Stack::sizing();
    std::string pre;   // weight-key prefix ("trk.", "dpt.<task>.")
    const char* name;  // the entry point, for error texts
    int rc = 0;
    bool dry = true;  // size query: no workspace, no weights, no launches - until on() gives the run a stream and memory

    Graph(const l4p_engine* e_, const char* name_, std::string pre_ = std::string())
        : e(e_), dt(e_->dtype), es(esize_of(e_->dtype)), pre(std::move(pre_)), name(name_) {}
    void on(l4p_stream stream, void* workspace, size_t bytes) {
        st = (hipStream_t)stream;
        ws = Stack::over(workspace, bytes);
        dry = false;
    }

    const void* W(const std::string& k) {
        if (dry) return (const void*)256;
        const void* p = e->find(pre + k);
        if (!p && !rc) {
            l4p_set_error("weight '%s%s' was never bound", pre.c_str(), k.c_str());
            rc = L4P_E_MISSING;
        }
        return p;
    }
    const float* Wf(const std::string& k) { return (const float*)W(k); }
    void* alloc(size_t bytes) {
        void* p = ws.take(bytes);
        if (!p && !rc) {
            l4p_set_error("%s: workspace too small", name);
            rc = L4P_E_INVALID;
        }
        return p;
    }
    float* f32(long long rows, long long cols) { return (float*)alloc((size_t)rows * cols * 4); }
    void* T(long long rows, long long cols) { return alloc((size_t)rows * cols * es); }

    template <class F>
    void launch(F&& f) {
        if (!rc && !dry) rc = f();
    }
    void gemm(int mode, const GemmParams& p) {  // mode: 0 dense, 1 conv 3x3x3, 2 sub-pixel conv
        launch([&] { return launch_gemm(dt, mode, p, st); });
    }
};
#endif
