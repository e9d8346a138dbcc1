// deform_tail_host.cpp -- the block merge's index arithmetic (d3ga_amd/csrc/deform_tail.h: deform_merge_put, deform_merge_items,
// deform_merge_sums) on the host, against a scalar reference.  A program of its own: built with -fsanitize=address,undefined by
// tests/test_deform_tail_host.py and run there; any read or write outside the planes, the plan or the partials ends it.
//
//   deform_tail_host P [P ...]      -> one line per P, exit status 0 when every partial equals the reference bit for bit
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../d3ga_amd/csrc/deform_tail.h"

using namespace d3ga;

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rndf() { return (float)(rnd() % 20001) / 10000.0f - 1.0f; }

static int check(int P) {
    const int V = std::max(4, P / 3 + 5);                       // few vertices: long segments, many Gaussians per vertex
    const int blocks = (P + kMergeBlock - 1) / kMergeBlock;
    // vertex of item 4 i + c (four distinct corners per Gaussian, neighbours share vertices)
    std::vector<int> vid(4 * (size_t)P);
    for (int i = 0; i < P; ++i) {
        const int base = (int)(rnd() % V);
        for (int c = 0; c < 4; ++c) vid[4 * (size_t)i + c] = (base + c * (1 + (int)(rnd() % 2))) % V;
    }
    // the plan, as cage_deform.py: merge_plan builds it: items of a block in (vertex, item) order; a segment = a run of one vertex
    std::vector<uint16_t> item_pos(4 * (size_t)P), seg_begin;
    std::vector<int32_t> seg_ptr(blocks + 1, 0), seg_vertex;
    for (int b = 0; b < blocks; ++b) {
        const int first = 4 * b * kMergeBlock, n = deform_merge_items(P, b);
        if (n != std::min(kMergeItems, 4 * P - first)) { std::printf("P=%d block %d: %d items\n", P, b, n); return 1; }
        std::vector<int> order(n);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return vid[first + x] < vid[first + y]; });
        for (int pos = 0; pos < n; ++pos) {
            item_pos[first + order[pos]] = (uint16_t)pos;
            if (pos == 0 || vid[first + order[pos]] != vid[first + order[pos - 1]]) {
                seg_begin.push_back((uint16_t)pos);
                seg_vertex.push_back(vid[first + order[pos]]);
            }
        }
        seg_ptr[b + 1] = (int32_t)seg_begin.size();
    }
    const size_t S = seg_begin.size();
    // exactly-sized heap blocks: the sanitizer sees an access one element outside any of them
    std::vector<float> partials(3 * S, -7.0f), want(3 * S, 0.0f);
    std::vector<DeformGrad> grads(P);
    for (int i = 0; i < P; ++i) {
        DeformGrad &o = grads[i];
        o.gx0 = v3(rndf(), rndf(), rndf()); o.gx1 = v3(rndf(), rndf(), rndf());
        o.gx2 = v3(rndf(), rndf(), rndf()); o.gx3 = v3(rndf(), rndf(), rndf());
    }
    const DeformMerge mg = {item_pos.data(), seg_ptr.data(), seg_begin.data(), partials.data()};
    auto *planes = reinterpret_cast<float (*)[3][kMergeItems]>(std::malloc(sizeof(float) * 3 * kMergeItems));
    for (int b = 0; b < blocks; ++b) {
        std::memset(planes, 0x7f, sizeof(float) * 3 * kMergeItems);          // garbage: every slot read must have been written
        for (int t = 0; t < kMergeBlock; ++t) {                               // the scatter of every live thread ...
            const int i = b * kMergeBlock + t;
            if (i >= P) continue;
            const uint16_t *ps = item_pos.data() + 4 * (size_t)i;
            deform_merge_put(*planes, ps[0], ps[1], ps[2], ps[3], grads[i]);
        }
        for (int t = 0; t < kMergeBlock; ++t) deform_merge_sums(*planes, mg, P, b, t);      // ... the barrier, every thread's sums
    }
    std::free(planes);
    // scalar reference: every segment's items in item order (the stable sort keeps it)
    for (int b = 0; b < blocks; ++b) {
        const int first = 4 * b * kMergeBlock, n = deform_merge_items(P, b);
        for (int g = seg_ptr[b]; g < seg_ptr[b + 1]; ++g)
            for (int k = 0; k < n; ++k) {
                if (vid[first + k] != seg_vertex[g]) continue;
                const DeformGrad &o = grads[(first + k) / 4];
                const V3 c = (k & 3) == 0 ? o.gx0 : (k & 3) == 1 ? o.gx1 : (k & 3) == 2 ? o.gx2 : o.gx3;
                want[3 * (size_t)g] += c.x; want[3 * (size_t)g + 1] += c.y; want[3 * (size_t)g + 2] += c.z;
            }
    }
    const bool same = std::memcmp(partials.data(), want.data(), sizeof(float) * 3 * S) == 0;
    std::printf("P=%d blocks=%d segments=%zu %s\n", P, blocks, S, same ? "ok" : "MISMATCH");
    return same ? 0 : 1;
}

int main(int argc, char **argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) bad |= check(std::atoi(argv[a]));
    return argc > 1 ? bad : 2;
}
