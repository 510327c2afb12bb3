// exact_grid.cpp -- a stand-alone program over fpng_amd/csrc/exact_grid.h for tests/test_exact_grid_cpu.py: the host forms of what
// the view-stage kernels and their launchers run.  Standard input, a command per line:
//   walk <limit> <block> <n> <pre[0]> .. <pre[n]>    exact_grid_walk (limit 0: the default, exact_grid_limit(block))
//       -> "walk <1|0> <pieces>" and per piece " <r0> <r1> <workgroups>"
//   find <n> <pre[0]> .. <pre[n]>                      exact_grid_find and exact_grid_within for every b < pre[n] - pre[0]
//       -> "find <count>" and per workgroup " <lo> <within>"
//   limit <block>                                      -> "limit <exact_grid_limit(block)>"
// Built with the address and undefined-behaviour sanitizers; pre[] is a heap array of exactly n + 1 words, so a read past it is seen.
#include "exact_grid.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace fpng_amd;

static bool read_pre(std::vector<uint64_t> &pre, unsigned long long n)
{
    pre.resize(n + 1);
    pre.shrink_to_fit();
    for (auto &v : pre) {
        unsigned long long x;
        if (scanf("%llu", &x) != 1) return false;
        v = x;
    }
    return true;
}

int main()
{
    char cmd[16];
    std::vector<uint64_t> pre;
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "walk")) {
            unsigned long long limit, block, n;
            if (scanf("%llu %llu %llu", &limit, &block, &n) != 3 || !read_pre(pre, n)) return 2;
            std::vector<unsigned long long> pieces;
            const auto launch = [&](uint32_t r0, uint32_t r1, uint32_t groups) { pieces.insert(pieces.end(), {r0, r1, groups}); };
            const bool ok = limit ? exact_grid_walk(pre.data(), (uint32_t)n, (uint32_t)block, launch, limit) : exact_grid_walk(pre.data(), (uint32_t)n, (uint32_t)block, launch);
            printf("walk %d %zu", ok ? 1 : 0, pieces.size() / 3);
            for (auto v : pieces) printf(" %llu", v);
            printf("\n");
        } else if (!strcmp(cmd, "find")) {
            unsigned long long n;
            if (scanf("%llu", &n) != 1 || !n || !read_pre(pre, n)) return 2;
            const uint64_t count = pre[n] - pre[0];
            printf("find %llu", (unsigned long long)count);
            for (uint64_t b = 0; b < count; b++) {
                uint64_t g;
                const uint32_t lo = exact_grid_find(pre.data(), (uint32_t)n, (uint32_t)b, g);
                printf(" %u %llu", lo, (unsigned long long)exact_grid_within(pre.data(), lo, g));
            }
            printf("\n");
        } else if (!strcmp(cmd, "limit")) {
            unsigned long long block;
            if (scanf("%llu", &block) != 1) return 2;
            printf("limit %llu\n", (unsigned long long)exact_grid_limit((uint32_t)block));
        } else
            return 2;
    }
    return 0;
}
