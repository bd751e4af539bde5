// The walk of `zot contigs` (zk_contig_walk, zotmer_amd/csrc/hostio.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer,
// on the CPU: a stand-alone program that replays a file of cases (tests/test_contig_walk_sanitizers.py writes it) and hands the
// walk heap blocks of exactly the advertised sizes -- next and rc of n entries, nodes of cap_nodes, offs of cap_contigs + 1 --
// so that an access one element past any of them ends the run.
//
//   contig_walk_san_driver <cases> <results>
// cases:   u64 words; per case  n, K, min_len, cap_nodes, cap_contigs, next[n], rc[n]
// results: u64 words; per case  the return code (as int64), n_nodes, n_contigs and, when the code is 0, nodes[n_nodes],
//          offs[n_contigs + 1]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../include/zotk.h"

static std::vector<uint64_t> read_words(const char* path) {
    std::vector<uint64_t> w;
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    uint64_t v;
    while (fread(&v, 8, 1, f) == 1) w.push_back(v);
    fclose(f);
    return w;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <cases> <results>\n", argv[0]); return 2; }
    const std::vector<uint64_t> in = read_words(argv[1]);
    std::vector<uint64_t> out;
    size_t at = 0, cases = 0;
    while (at < in.size()) {
        if (in.size() - at < 5) { fprintf(stderr, "a case header is cut short\n"); return 2; }
        const uint64_t n = in[at], K = in[at + 1], min_len = in[at + 2], cap_nodes = in[at + 3], cap_contigs = in[at + 4];
        at += 5;
        if (in.size() - at < 2 * n) { fprintf(stderr, "a case is cut short\n"); return 2; }
        uint32_t* next = new uint32_t[n];
        uint32_t* rc = new uint32_t[n];
        for (uint64_t i = 0; i < n; i++) { next[i] = (uint32_t)in[at + i]; rc[i] = (uint32_t)in[at + n + i]; }
        at += 2 * n;
        uint32_t* nodes = new uint32_t[cap_nodes];
        uint64_t* offs = new uint64_t[cap_contigs + 1];
        uint64_t nn = 0, nc = 0;
        const int r = zk_contig_walk(next, rc, n, (int)(int64_t)K, min_len, nodes, cap_nodes, offs, cap_contigs, &nn, &nc);
        out.push_back((uint64_t)(int64_t)r);
        out.push_back(nn);
        out.push_back(nc);
        if (r == ZK_OK) {
            for (uint64_t i = 0; i < nn; i++) out.push_back(nodes[i]);
            for (uint64_t i = 0; i <= nc; i++) out.push_back(offs[i]);
        }
        delete[] next;
        delete[] rc;
        delete[] nodes;
        delete[] offs;
        cases++;
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (!out.empty() && fwrite(out.data(), 8, out.size(), f) != out.size()) { perror("write"); return 2; }
    fclose(f);
    printf("cases %zu\n", cases);
    return 0;
}
