// Standalone timing / tracing of the encoder attention kernels (csrc/attention.hip, csrc/attention64.hip) with parts disabled
// (-DATTN_DBG_* / -DATTN64_DBG_*: wrong results) and, with -DATTN64_TRACE, the s_memtime stamps of wave 0 of workgroup 0 of the
// 64-row kernel at the phase boundaries of every KV step.  tools/probes/build_attn.sh and build_attn64.sh build the variants.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form=1 -I include -I l4p_amd/csrc [-D...] tools/probes/attn_probe.hip -o ...
//   attn_probe [batch] ["form"] [--zeros]
// S = 2048, H = 16, Dh = 88, bf16, q pre-scaled (the engine's launch: bf16 with the scale inside would get the compiler-scheduled body).
// form: a tag of attn_form_tag ("kvsplit", "unsplit", "qsplit persist", "qsplit pertile", "rows64", "unsplit cs", "kvsplit cs");
// default: what attn_select gives the engine at that batch.  --zeros: all-zero operands, the same instruction stream at the clock an
// idle matrix pipe is granted.
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>
bool g_prof_on = false;
void prof_begin(int, hipStream_t, const char*) {}
void prof_end(int, hipStream_t) {}
void l4p_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }
#ifndef ATTN_PROBE_BATCH
#define ATTN_PROBE_BATCH 1  // (build_attn64.sh: 4)
#endif
int knob(int) { return 1; }  // (launch_attention's snapshot; the probe calls launch_attn_form itself)
#include "../../l4p_amd/csrc/attention.hip"
#include "../../l4p_amd/csrc/attention64.hip"

int main(int argc, char** argv) {
    int B = 0;
    const char* want = nullptr;
    bool zeros = false;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--zeros")) zeros = true;
        else if (!B && atoi(argv[i]) > 0) B = atoi(argv[i]);
        else want = argv[i];
    }
    if (!B) B = ATTN_PROBE_BATCH;
    const int S = 2048, H = 16, Dh = 88;
    // the first knob setting (defaults first) under which attn_select gives this launch the form asked for
    AttnChoice c = {};
    const char* err = "";
    bool found = false;
    for (int a = 1; a >= 0 && !found; --a)
        for (int v = 0; v < 3 && !found; ++v)
            for (int p = 1; p >= 0 && !found; --p) {
                c = attn_select(L4P_BF16, B, S, H, Dh, L4P_ATTN_PRESCALED, AttnKnobs{v, p, a}, &err);
                found = !want || !strcmp(want, attn_form_tag(c));
            }
    if (!found) {
        fprintf(stderr, "no knob setting gives form '%s' at batch %d\n", want, B);
        return 2;
    }
    const size_t n = (size_t)B * S * H * ATTN_DP;
    std::vector<unsigned short> h(n);
    // roughly N(0,1) bf16 values (sum of 12 uniforms - 6 from an LCG): realistic score statistics for the softmax path
    unsigned st = 12345u;
    for (size_t i = 0; i < n; ++i) {
        float acc = -6.f;
        for (int k = 0; k < 12; ++k) {
            st = st * 1664525u + 1013904223u;
            acc += (st >> 8) * (1.0f / 16777216.0f);
        }
        unsigned u;
        memcpy(&u, &acc, 4);
        h[i] = zeros ? 0 : (unsigned short)((u + 0x8000u) >> 16);
    }
    void *q, *kt, *vt, *out;
    hipMalloc(&q, n * 2); hipMalloc(&kt, n * 2); hipMalloc(&vt, n * 2); hipMalloc(&out, n * 2);
    hipMemcpy(q, h.data(), n * 2, hipMemcpyHostToDevice);
    hipMemcpy(kt, h.data(), n * 2, hipMemcpyHostToDevice);
    hipMemcpy(vt, h.data(), n * 2, hipMemcpyHostToDevice);
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    for (int i = 0; i < 5; ++i)
        if (launch_attn_form(L4P_BF16, c, q, kt, vt, out, B, S, H, Dh, 0)) return 1;
    hipEventRecord(a, 0);
    const int it = 50;
    for (int i = 0; i < it; ++i) launch_attn_form(L4P_BF16, c, q, kt, vt, out, B, S, H, Dh, 0);
    hipEventRecord(b, 0); hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b);
    printf("B=%d %s (grid %d x %d, %d B LDS)%s: %.2f us per launch\n", B, attn_form_tag(c), c.grid, c.block, c.lds_bytes, zeros ? " zeros" : "", ms / it * 1e3);
#ifdef ATTN64_TRACE
    if (c.form != ATTN_ROWS64) return 0;
    std::vector<long long> t(4096);
    hipMemcpyFromSymbol(t.data(), HIP_SYMBOL(attn64::g_trace), 4096 * 8);
    printf("tile 0: prologue %lld  loop %lld  store %lld | tile 1: prologue %lld loop %lld store %lld (cycles)\n", t[1] - t[0], t[2] - t[1],
           t[3] - t[2], t[5] - t[4], t[6] - t[5], t[7] - t[6]);
    long long sum[6] = {};
    for (int i = 2; i < 30; ++i) {  // steady-state steps of the LAST tile walked (stamps are overwritten tile after tile)
        const long long* s = &t[8 + i * 8];
        const long long d[6] = {s[1] - s[0], s[2] - s[1], s[3] - s[2], s[4] - s[3], s[5] - s[4], t[8 + (i + 1) * 8] - s[0]};
        for (int k = 0; k < 6; ++k) sum[k] += d[k];
        if (i < 8) printf("step %2d: dma %lld  rare-check %lld  QK phase %lld  PV phase %lld  barrier %lld | step %lld\n", i, d[0], d[1], d[2], d[3], d[4], d[5]);
    }
    printf("mean of steps 2..29: dma %.0f  check %.0f  QK %.0f  PV %.0f  barrier %.0f | step %.0f (48 MFMAs = 1536 cycles)\n", sum[0] / 28.0, sum[1] / 28.0,
           sum[2] / 28.0, sum[3] / 28.0, sum[4] / 28.0, sum[5] / 28.0);
#endif
    return 0;
}
