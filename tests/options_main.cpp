// The switch table as the parser (chatllm.cpp_amd/csrc/options.cpp) reads THIS process's environment: warnings on stderr, cllm_options_describe's text on stdout.
// tests/test_options.py builds it from the parser alone with -fsanitize=address,undefined and runs it once per case.
#include "../chatllm.cpp_amd/csrc/options.h"

#include <stdio.h>
#include <string.h>
#include <vector>

int main() {
    const size_t n = opt_describe(nullptr, 0);
    std::vector<char> all(n + 1);
    if (opt_describe(all.data(), all.size()) != n || strlen(all.data()) != n) return 2;
    char cut[17];                                       // a short buffer is filled to its end and terminated, never overrun
    if (opt_describe(cut, sizeof(cut)) != n || strlen(cut) != 16 || memcmp(cut, all.data(), 16)) return 3;
    fputs(all.data(), stdout);
    return 0;
}
