// tools/link_vanishing_bench.hip -- Z_D(eta) of K proof links: the library's wave-per-link kernel (csrc/verifier.cuh,
// vfy_link_vanishing_kernel) against a thread-per-link variant kept HERE only, for the measurement DESIGN.md section 4.14 quotes.
// Alternating launches in one process on one card, every time listed; the two kernels' outputs are compared bit for bit.
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off tools/link_vanishing_bench.hip -o tools/link_vanishing_bench
// Run:   tools/link_vanishing_bench [K = 256] [size = 1024] [rounds = 21]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../mpc-jellyfish_amd/csrc/verifier.cuh"
using namespace mzk;

#define CHECK(e)                                                                              \
    do {                                                                                      \
        const hipError_t r_ = (e);                                                            \
        if (r_ != hipSuccess) { std::printf("%s: %s\n", #e, hipGetErrorString(r_)); std::exit(1); } \
    } while (0)

// the variant: one THREAD per link walks the size factors as one dependent chain (the reference's loop, proof_linking.rs:162-176)
template <class P>
__global__ __launch_bounds__(VFY_THREADS) void thread_per_link_kernel(unsigned long long K, const unsigned long long* __restrict__ layouts,
                                                                      const uint32_t* __restrict__ eta, uint32_t* __restrict__ vanish,
                                                                      uint32_t* __restrict__ proof_rows) {
    using F = Fp<P>;
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    const unsigned long long alignment = layouts[3 * i], offset = layouts[3 * i + 1], size = layouts[3 * i + 2];
    const F x = load_fp<P>(eta + i * 8ull);
    F g = F::from_const(P::ROOT);
    for (int k = (int)alignment; k < P::TWO_ADICITY; k++) g = sqr(g);
    F root = F::one();
    {
        F b = g;
        for (unsigned long long e = offset & ((1ull << alignment) - 1); e; e >>= 1) {
            if (e & 1) root = root * b;
            b = sqr(b);
        }
    }
    F z = F::one();
    for (unsigned long long k = 0; k < size; k++) {
        z = z * (x - root);
        root = root * g;
    }
    store_fp<P>(vanish + i * 8ull, z);
    uint32_t* row = proof_rows + i * 4 * 8ull;
    store_fp<P>(row, F::one());
    store_fp<P>(row + 8, neg(F::one()));
    store_fp<P>(row + 16, neg(z));
    store_fp<P>(row + 24, x);
}

template <class P>
void run(const char* name, unsigned long long K, unsigned long long size, int rounds) {
    std::vector<unsigned long long> layouts(3 * K);
    std::vector<uint32_t> eta(8 * K);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    const auto next = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (unsigned long long i = 0; i < K; i++) {
        layouts[3 * i] = 12, layouts[3 * i + 1] = next() % 3000, layouts[3 * i + 2] = size;
        for (int k = 0; k < 8; k++) eta[8 * i + k] = (uint32_t)next();
        eta[8 * i + 7] &= 0x0FFFFFFFu;                                 // below both moduli: a field element in Montgomery form
    }
    unsigned long long* d_lay;
    uint32_t *d_eta, *d_van[2], *d_rows[2];
    CHECK(hipMalloc(&d_lay, K * 24));
    CHECK(hipMalloc(&d_eta, K * 32));
    for (int v = 0; v < 2; v++) { CHECK(hipMalloc(&d_van[v], K * 32)); CHECK(hipMalloc(&d_rows[v], K * 128)); }
    CHECK(hipMemcpy(d_lay, layouts.data(), K * 24, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_eta, eta.data(), K * 32, hipMemcpyHostToDevice));
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    const auto launch = [&](int v) {
        if (v == 0) hipLaunchKernelGGL((vfy_link_vanishing_kernel<P>), dim3((unsigned)K), dim3(VFY_THREADS), 0, nullptr, d_lay, d_eta, d_van[0], d_rows[0]);
        else hipLaunchKernelGGL((thread_per_link_kernel<P>), dim3((unsigned)((K + VFY_THREADS - 1) / VFY_THREADS)), dim3(VFY_THREADS), 0, nullptr, K, d_lay, d_eta,
                                d_van[1], d_rows[1]);
    };
    std::vector<float> t[2];
    for (int r = 0; r < rounds + 2; r++)                              // two warm-up rounds, then alternating
        for (int v = 0; v < 2; v++) {
            CHECK(hipEventRecord(a, nullptr));
            launch(v);
            CHECK(hipEventRecord(b, nullptr));
            CHECK(hipEventSynchronize(b));
            CHECK(hipGetLastError());
            float ms = 0;
            CHECK(hipEventElapsedTime(&ms, a, b));
            if (r >= 2) t[v].push_back(ms);
        }
    std::vector<uint32_t> out[2];
    for (int v = 0; v < 2; v++) {
        out[v].resize(K * 8 + K * 32);
        CHECK(hipMemcpy(out[v].data(), d_van[v], K * 32, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(out[v].data() + K * 8, d_rows[v], K * 128, hipMemcpyDeviceToHost));
    }
    const bool same = out[0] == out[1];
    static const char* const NAMES[2] = {"wave per link  ", "thread per link"};
    std::printf("%s  K = %llu links of size %llu, %d alternating rounds; outputs %s\n", name, K, size, rounds, same ? "identical" : "DIFFER");
    for (int v = 0; v < 2; v++) {
        std::vector<float> sorted = t[v];
        std::sort(sorted.begin(), sorted.end());
        std::printf("  %s  median %8.3f ms  min %8.3f  max %8.3f  all:", NAMES[v], sorted[sorted.size() / 2], sorted.front(), sorted.back());
        for (float x : t[v]) std::printf(" %.3f", x);
        std::printf("\n");
    }
    if (!same) std::exit(2);
    CHECK(hipFree(d_lay));
    CHECK(hipFree(d_eta));
    for (int v = 0; v < 2; v++) { CHECK(hipFree(d_van[v])); CHECK(hipFree(d_rows[v])); }
}

int main(int argc, char** argv) {
    const unsigned long long K = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 256, size = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1024;
    const int rounds = argc > 3 ? std::atoi(argv[3]) : 21;
    if (!K || K > (1u << 20) || size > (1ull << 27) || rounds < 1) { std::printf("bad arguments\n"); return 1; }
    run<BlsFr>("BLS12-381", K, size, rounds);
    run<BnFr>("BN254    ", K, size, rounds);
    return 0;
}
