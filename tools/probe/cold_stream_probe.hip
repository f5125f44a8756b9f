// Dev probe (round 6): what bounds a SHORT streaming launch on operands that are not cache-resident?
//
// profiles/r06_hbm_cold_stream.md: a torch element-wise pass over 64 MB in + 64 MB out takes 19.6 us when its operands sit in the
// memory-side cache and 34.8 us behind a 1-GB evicting pass (3.85 TB/s) -- and the step's large launches all sit at 3 - 3.9 TB/s of
// moved bytes.  If that ceiling is Little's law (bytes in flight per CU x HBM latency) rather than the memory system, more
// independent loads per lane must lift it.  This probe times, with device timestamps (first workgroup in -> last workgroup out),
//   copy<U>   : U independent 16-byte loads per lane, then U stores, one pass per workgroup (grid = n / (256 U))
//   copyP<U>  : the same body as a persistent grid-stride loop (256 CUs x 8 workgroups)
//   read<U>   : loads only (a sum per lane, one store per workgroup)
// hot (same buffers again), cold behind a READ of 1 GB, cold behind a FILL of 1 GB (dirty lines in the memory-side cache).
//   hipcc --offload-arch=gfx950 -O3 -o tools/probe/cold_stream_probe.bin tools/probe/cold_stream_probe.hip
// `cold_stream_probe.bin store` runs the store-policy section instead (below; tools/probe/store_policy_probe.sh, profiles/store_policy_probe.txt).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define CK(x)                                                                             \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } \
    } while (0)

struct Stamp { unsigned long long t0, t1; };
// one pair per workgroup, reduced on the host (atomics on one address serialise the workgroups: 11 ns each)
__device__ __forceinline__ void stamp_in(Stamp* s) {
    if (threadIdx.x == 0) s[blockIdx.x].t0 = wall_clock64();
}
__device__ __forceinline__ void stamp_out(Stamp* s) {
    __syncthreads();
    if (threadIdx.x == 0) s[blockIdx.x].t1 = wall_clock64();
}

template <int U> __global__ __launch_bounds__(256) void k_copy(const float4* __restrict__ a, float4* __restrict__ b, size_t n16, Stamp* s) {
    stamp_in(s);
    const size_t base = (size_t)blockIdx.x * 256 * U + threadIdx.x;
    float4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = a[base + (size_t)u * 256];
#pragma unroll
    for (int u = 0; u < U; ++u) b[base + (size_t)u * 256] = v[u];
    stamp_out(s);
}
template <int U> __global__ __launch_bounds__(256) void k_copy_p(const float4* __restrict__ a, float4* __restrict__ b, size_t n16, Stamp* s) {
    stamp_in(s);
    const size_t step = (size_t)gridDim.x * 256 * U;
    for (size_t base = (size_t)blockIdx.x * 256 * U + threadIdx.x; base < n16; base += step) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = a[base + (size_t)u * 256];
#pragma unroll
        for (int u = 0; u < U; ++u) b[base + (size_t)u * 256] = v[u];
    }
    stamp_out(s);
}
template <int U> __global__ __launch_bounds__(256) void k_read(const float4* __restrict__ a, float* __restrict__ out, size_t n16, Stamp* s) {
    stamp_in(s);
    const size_t base = (size_t)blockIdx.x * 256 * U + threadIdx.x;
    float4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = a[base + (size_t)u * 256];
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) acc += v[u].x + v[u].y + v[u].z + v[u].w;
    if (acc == 12345.678f) out[blockIdx.x] = acc;
    stamp_out(s);
}
__global__ __launch_bounds__(256) void k_evict_read(const float4* __restrict__ a, float* out, size_t n16) {
    float acc = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) { const float4 v = a[i];  acc += v.x + v.w; }
    if (acc == 12345.678f) out[0] = acc;
}
__global__ __launch_bounds__(256) void k_evict_fill(float4* __restrict__ a, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) a[i] = make_float4(1.f, 2.f, 3.f, 4.f);
}

static float4 *g_big, *g_a, *g_b;
static float* g_out;
static Stamp* g_s;
static size_t g_big16;

enum Mode { HOT, COLD_R, COLD_W };
constexpr unsigned kMaxBlocks = 1u << 16;
template <typename F> static double run(Mode m, unsigned blocks, F launch) {
    std::vector<double> us;
    static std::vector<Stamp> h(kMaxBlocks);
    for (int it = 0; it < 9; ++it) {
        if (m == COLD_R) hipLaunchKernelGGL(k_evict_read, dim3(4096), dim3(256), 0, 0, g_big, g_out, g_big16);
        if (m == COLD_W) hipLaunchKernelGGL(k_evict_fill, dim3(4096), dim3(256), 0, 0, g_big, g_big16);
        launch();
        CK(hipMemcpy(h.data(), g_s, sizeof(Stamp) * blocks, hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ull, t1 = 0;
        for (unsigned b = 0; b < blocks; ++b) { t0 = std::min(t0, h[b].t0);  t1 = std::max(t1, h[b].t1); }
        if (it >= 2) us.push_back((double)(t1 - t0) * 0.01);          // wall_clock64: 100 MHz
    }
    std::sort(us.begin(), us.end());
    return us[us.size() / 2];
}

template <int U> static void row(size_t mb) {
    const size_t n16 = mb * 1024 * 1024 / 16;
    const unsigned grid = (unsigned)(n16 / (256 * U));
    double c[3], p[3], r[3];
    for (int m = 0; m < 3; ++m) {
        c[m] = run((Mode)m, grid, [&] { hipLaunchKernelGGL(k_copy<U>, dim3(grid), dim3(256), 0, 0, g_a, g_b, n16, g_s); });
        p[m] = run((Mode)m, 2048, [&] { hipLaunchKernelGGL(k_copy_p<U>, dim3(2048), dim3(256), 0, 0, g_a, g_b, n16, g_s); });
        r[m] = run((Mode)m, grid, [&] { hipLaunchKernelGGL(k_read<U>, dim3(grid), dim3(256), 0, 0, g_a, g_out, n16, g_s); });
    }
    const double mbs = mb * 1.048576;
    auto f = [&](double us, double mult) { static char buf[16][48]; static int k = 0; char* o = buf[k++ & 15]; snprintf(o, 48, "%6.2f (%4.2f)", us, mult * mbs / us); return o; };
    printf("| %3zu MB | %2d | %s | %s | %s | %s | %s | %s | %s | %s | %s |\n", mb, U, f(c[0], 2), f(c[1], 2), f(c[2], 2), f(p[0], 2), f(p[1], 2), f(p[2], 2),
           f(r[0], 1), f(r[1], 1), f(r[2], 1));
}

// ---- store-policy section (`cold_stream_probe.bin store`): what does the FLAVOUR of a producer's stores cost the launch behind it?
// The producer writes B bytes of 512-byte rows, 16 bytes per lane (a half-wave per row), in one of five flavours; a follower is launched
// behind it on the same stream with nothing in between:
//   (i)   read    : a read-only pass over ANOTHER buffer of B bytes
//   (ii)  consume : a read-only pass over what the producer wrote (the next-launch consumer)
//   (iii) gather  : 131072 half-wave gathers of 512-byte rows from a 13.6-MB table (the attention launches' access); the table is read
//                   once between the background and the producer, so it is what a projection launch would have left behind
// Every case runs behind 300 MB of plain writes (the state the training step leaves the memory-side cache in).  Reported: producer
// duration, boundary (producer's last workgroup out -> follower's first workgroup in), follower duration; median of 7 [min .. max].
// The sc1 forms are raw-buffer stores with the cache-policy argument (compiler-tracked: the compiler counts vmcnt itself); aux bits on
// gfx950: 1 = sc0, 2 = nt, 16 = sc1.
typedef float pf4 __attribute__((ext_vector_type(4)));
enum Flavour { F_PLAIN = 0, F_NT = 2, F_SC1 = 16, F_SC0SC1 = 17, F_NTSC1 = 18 };
template <int F> __device__ __forceinline__ void store16(pf4* base, __amdgpu_buffer_rsrc_t rs, size_t i, pf4 v) {
    if constexpr (F == F_PLAIN) base[i] = v;
    else if constexpr (F == F_NT) __builtin_nontemporal_store(v, &base[i]);
    else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(16))) unsigned, v), rs, (int)(i * 16), 0, F);
}
// one pass per workgroup (grid = n16 / 1024: four stores per lane) or, with a smaller grid, a persistent grid-stride stream
template <int F> __global__ __launch_bounds__(256) void k_prod(pf4* __restrict__ b, size_t n16, Stamp* s) {
    stamp_in(s);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(b, 0, (int)(n16 * 16), 0x00020000);
    const size_t step = (size_t)gridDim.x * 1024;
    for (size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x; base < n16; base += step) {
        const float f = (float)(base & 1023);
#pragma unroll
        for (int u = 0; u < 4; ++u) store16<F>(b, rs, base + (size_t)u * 256, (pf4){f, 1.f, 2.f, (float)u});
    }
    stamp_out(s);
}
// 8 rows per half-wave and workgroup pass; the row index is near the reader's own position (a molecule's rows are neighbours) with a hashed offset
__global__ __launch_bounds__(256) void k_gather(const float4* __restrict__ tab, unsigned rows, float* __restrict__ out, Stamp* s) {
    stamp_in(s);
    const unsigned hw = (blockIdx.x * 256 + threadIdx.x) >> 5, lane = threadIdx.x & 31, nhw = gridDim.x * 8;
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const unsigned q = hw * 8 + u;
        const unsigned r = (unsigned)(((unsigned long long)hw * rows) / nhw + ((q * 2654435761u) >> 26)) % rows;
        v[u] = tab[(size_t)r * 32 + lane];
    }
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u].x + v[u].y + v[u].z + v[u].w;
    if (acc == 12345.678f) out[blockIdx.x] = acc;
    stamp_out(s);
}

struct Med { double med, lo, hi; };
static Med med_of(std::vector<double>& v) { std::sort(v.begin(), v.end());  return {v[v.size() / 2], v.front(), v.back()}; }
static void span(const Stamp* h, unsigned blocks, unsigned long long& t0, unsigned long long& t1) {
    t0 = ~0ull; t1 = 0;
    for (unsigned b = 0; b < blocks; ++b) { t0 = std::min(t0, h[b].t0);  t1 = std::max(t1, h[b].t1); }
}
constexpr size_t kBgBytes = (size_t)300 << 20, kTabRows = 26562;      // 26562 rows of 512 B = 13.6 MB
static float4* g_tab;
static Stamp* g_s2;
template <int F> static void launch_prod(size_t n16, unsigned grid) { hipLaunchKernelGGL(k_prod<F>, dim3(grid), dim3(256), 0, 0, (pf4*)g_b, n16, g_s); }
static void launch_flavour(int f, size_t n16, unsigned grid) {
    switch (f) {
        case F_PLAIN: launch_prod<F_PLAIN>(n16, grid); break;
        case F_NT: launch_prod<F_NT>(n16, grid); break;
        case F_SC1: launch_prod<F_SC1>(n16, grid); break;
        case F_SC0SC1: launch_prod<F_SC0SC1>(n16, grid); break;
        default: launch_prod<F_NTSC1>(n16, grid); break;
    }
}
// follower: 0 read another buffer, 1 read the producer's, 2 gather, -1 none (producer alone)
static void store_case(int f, size_t mb, unsigned pgrid, int follower, Med& prod, Med& gap, Med& fol) {
    const size_t n16 = mb * 1024 * 1024 / 16;
    const unsigned rgrid = (unsigned)(n16 / 1024), ggrid = 2048, fgrid = follower == 2 ? ggrid : rgrid;
    static std::vector<Stamp> hp(kMaxBlocks), hf(kMaxBlocks);
    std::vector<double> vp, vg, vf;
    for (int it = 0; it < 9; ++it) {
        hipLaunchKernelGGL(k_evict_fill, dim3(4096), dim3(256), 0, 0, g_big, kBgBytes / 16);
        if (follower == 2) hipLaunchKernelGGL(k_evict_read, dim3(2048), dim3(256), 0, 0, g_tab, g_out, kTabRows * 32);
        launch_flavour(f, n16, pgrid);
        if (follower == 0) hipLaunchKernelGGL(k_read<4>, dim3(rgrid), dim3(256), 0, 0, g_a, g_out, n16, g_s2);
        if (follower == 1) hipLaunchKernelGGL(k_read<4>, dim3(rgrid), dim3(256), 0, 0, g_b, g_out, n16, g_s2);
        if (follower == 2) hipLaunchKernelGGL(k_gather, dim3(ggrid), dim3(256), 0, 0, g_tab, (unsigned)kTabRows, g_out, g_s2);
        CK(hipMemcpy(hp.data(), g_s, sizeof(Stamp) * pgrid, hipMemcpyDeviceToHost));
        unsigned long long p0, p1, f0 = 0, f1 = 0;
        span(hp.data(), pgrid, p0, p1);
        if (follower >= 0) { CK(hipMemcpy(hf.data(), g_s2, sizeof(Stamp) * fgrid, hipMemcpyDeviceToHost));  span(hf.data(), fgrid, f0, f1); }
        if (it < 2) continue;
        vp.push_back((double)(p1 - p0) * 0.01);
        if (follower >= 0) { vg.push_back(((double)f0 - (double)p1) * 0.01);  vf.push_back((double)(f1 - f0) * 0.01); }
    }
    prod = med_of(vp);
    if (follower >= 0) { gap = med_of(vg);  fol = med_of(vf); }
}
static int store_main() {
    static const struct { int f; const char* name; } fl[] = {{F_PLAIN, "plain"}, {F_NT, "nt"}, {F_SC1, "sc1"}, {F_SC0SC1, "sc0 sc1"}, {F_NTSC1, "nt sc1"}};
    static const char* fname[] = {"read other", "consume", "gather 13.6 MB"};
    CK(hipMalloc(&g_tab, kTabRows * 512));
    CK(hipMalloc(&g_s2, sizeof(Stamp) * kMaxBlocks));
    CK(hipMemset(g_tab, 0, kTabRows * 512));
    printf("store-policy probe: us, device timestamps, median of 7 [min .. max]; every case behind 300 MB of plain writes\n");
    printf("producer: 16-byte stores, 512-byte rows, one pass per workgroup (grid = B / 16 KB); boundary = producer's last workgroup out -> follower's first in\n");
    printf("| B | flavour | follower | producer | boundary | follower | boundary + follower |\n|---|---|---|---|---|---|---|\n");
    for (size_t mb : {16, 32, 64})
        for (int fo = 0; fo < 3; ++fo)
            for (auto& x : fl) {
                Med p, g, f;
                store_case(x.f, mb, (unsigned)(mb * 64), fo, p, g, f);
                printf("| %2zu MB | %-7s | %-14s | %6.2f [%6.2f .. %6.2f] | %5.2f [%5.2f .. %5.2f] | %6.2f [%6.2f .. %6.2f] | %6.2f |\n", mb, x.name, fname[fo], p.med,
                       p.lo, p.hi, g.med, g.lo, g.hi, f.med, f.lo, f.hi, g.med + f.med);
            }
    printf("\nproducer as a 256-workgroup persistent stream (one workgroup per CU), alone and with the read-other follower\n");
    printf("| B | flavour | producer alone (TB/s) | producer | boundary | follower |\n|---|---|---|---|---|---|\n");
    for (size_t mb : {16, 32, 64})
        for (auto& x : fl) {
            Med pa, p, g, f;
            store_case(x.f, mb, 256, -1, pa, g, f);
            store_case(x.f, mb, 256, 0, p, g, f);
            printf("| %2zu MB | %-7s | %6.2f [%6.2f .. %6.2f] (%4.2f) | %6.2f [%6.2f .. %6.2f] | %5.2f [%5.2f .. %5.2f] | %6.2f [%6.2f .. %6.2f] |\n", mb, x.name, pa.med, pa.lo,
                   pa.hi, mb * 1.048576 / pa.med, p.med, p.lo, p.hi, g.med, g.lo, g.hi, f.med, f.lo, f.hi);
        }
    return 0;
}

int main(int argc, char** argv) {
    const bool store = argc > 1 && std::string(argv[1]) == "store";
    g_big16 = (size_t)1024 * 1024 * 1024 / 16;
    CK(hipMalloc(&g_big, g_big16 * 16));
    CK(hipMalloc(&g_a, (size_t)128 << 20));
    CK(hipMalloc(&g_b, (size_t)128 << 20));
    CK(hipMalloc(&g_out, 1 << 22));
    CK(hipMalloc(&g_s, sizeof(Stamp) * kMaxBlocks));
    CK(hipMemset(g_big, 0, g_big16 * 16));
    CK(hipMemset(g_a, 0, (size_t)128 << 20));
    CK(hipMemset(g_b, 0, (size_t)128 << 20));
    if (store) return store_main();
    printf("us (TB/s moved), device timestamps first workgroup in -> last out, median of 7; U = independent 16-byte loads per lane\n");
    printf("| size (in; copy: + out) | U | copy hot | copy cold(read-evicted) | copy cold(fill-evicted) | persistent copy hot | cold(r) | cold(w) | read hot | cold(r) | cold(w) |\n");
    printf("|---|---|---|---|---|---|---|---|---|---|---|\n");
    for (size_t mb : {32, 64, 128}) {
        row<1>(mb);
        row<2>(mb);
        row<4>(mb);
        row<8>(mb);
        row<16>(mb);
    }
    return 0;
}
