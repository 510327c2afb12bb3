// lanes_rule.cpp -- prints fpng_amd::lanes_for() (fpng_amd/csrc/lanes.h) for the cases tests/test_abi.py checks, one per line:
// "<hardware queues> <FPNG_AMD_LANES or -> <lanes>".  Host-only: built with the system's C++ compiler, no HIP.
#include "lanes.h"

#include <cstdio>

int main()
{
    const int queues[] = {1, 2, 4, 7, 8, 16};
    const char *env[] = {nullptr, "1", "3", "8", "0", "12"};
    for (int q : queues)
        for (const char *e : env)
            printf("%d %s %u\n", q, e ? e : "-", fpng_amd::lanes_for(q, e, 8));
    return 0;
}
