// Host check of the running-sum RK stages (x3d2_amd/time_integrator.py, _runsum_stage): the final combination of a step
//     u = ((base + c1 d1) + c2 d2) + c3 d3,        each term  r = c * x + r  contracted to one fused multiply-add
// (k_lincomb and the term loop of k_ytile_transeq3<EPI>, compiled with -ffp-contract=fast), evaluated in one go and through
// partial sums that are STORED as a field and picked up by a later call, gives the same bits: a stored double is the
// value the chain carries, nothing is rounded twice.  Doubles and floats, random data of mixed magnitude.
//
//   c++ -O2 -std=c++17 -ffp-contract=fast -mfma -fsanitize=address,undefined tools/rk_chain_bits.cpp -o rk_chain_bits
//   ./rk_chain_bits            (no GPU needed; prints the counts, exit status 1 on any difference)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

// one term of the chain over a whole field, as its own "kernel": out may be in (in place), noinline so that the partial
// sum really goes through memory between two calls
template <class T>
__attribute__((noinline)) void term(std::vector<T> &out, const std::vector<T> &in, T c, const std::vector<T> &x)
{
    for (size_t i = 0; i < in.size(); i++) out[i] = c * x[i] + in[i];
}

template <class T>
__attribute__((noinline)) void chain3(std::vector<T> &u, const std::vector<T> &base, const T c[3],
                                      const std::vector<T> *d[3])
{
    for (size_t i = 0; i < base.size(); i++) {
        T r = base[i];
        for (int k = 0; k < 3; k++) r = c[k] * (*d[k])[i] + r;
        u[i] = r;
    }
}

template <class T, class U>
long run(const char *name, uint64_t seed)
{
    const size_t n = 1 << 16;
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> g(0.0, 1.0);
    std::uniform_int_distribution<int> ex(-12, 12);
    auto fill = [&](std::vector<T> &v) {
        for (auto &x : v) x = (T)std::ldexp(g(rng), ex(rng));
    };
    std::vector<T> base(n), d1(n), d2(n), d3(n), u(n), e(n), v(n);
    fill(base); fill(d1); fill(d2); fill(d3);
    const T dt = (T)1e-3, c[3] = {(T)(2.0 / 9.0) * dt, (T)(1.0 / 3.0) * dt, (T)(4.0 / 9.0) * dt};  // RK3's b dt
    const std::vector<T> *d[3] = {&d1, &d2, &d3};
    chain3(u, base, c, d);       // in one go
    term(e, base, c[0], d1);     // stage 1: e1 = base + b1 dt d1, a field of its own
    term(e, e, c[1], d2);        // stage 2: in place
    term(v, e, c[2], d3);        // stage 3: u = e2 + b3 dt d3
    long diff = 0;
    for (size_t i = 0; i < n; i++) {
        U a, b;
        std::memcpy(&a, &u[i], sizeof(U));
        std::memcpy(&b, &v[i], sizeof(U));
        diff += a != b;
    }
    std::printf("%s: %zu values, %ld differ\n", name, n, diff);
    return diff;
}

int main()
{
    long diff = 0;
    for (uint64_t seed = 1; seed <= 4; seed++) {
        diff += run<double, uint64_t>("double", seed);
        diff += run<float, uint32_t>("float", 100 + seed);
    }
    std::printf(diff ? "FAILED\n" : "equal bits\n");
    return diff ? 1 : 0;
}
