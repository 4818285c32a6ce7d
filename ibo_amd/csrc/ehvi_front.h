// ehvi_front.h -- the canonical form of a two-objective Pareto front for the expected hypervolume improvement (abi_ehvi.hip).  Host code
// only, no HIP and nothing of the library behind it: a stand-alone program can include it and run it under a sanitizer.
#pragma once
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#define IBO_EHVI_FRONT_OK        0
#define IBO_EHVI_FRONT_BAD_REF   1      // a NaN or an infinity in the reference point
#define IBO_EHVI_FRONT_BAD_POINT 2      // a NaN or an infinity in the front (*where: its row)
#define IBO_EHVI_FRONT_TOO_MANY  3      // more than max_points left (*where: how many)

// front: nfront x 2 row-major, both objectives to be maximised; ref[2].  Points not strictly above ref in both coordinates, dominated
// points and duplicates go; the rest comes out as interleaved (a_i, b_i), a strictly ascending and b strictly descending.
static inline int ehvi_canonical_front(int nfront, const double *front, const double *ref, int max_points, std::vector<double> *out,
                                       long long *where)
{
    out->clear();
    if (!std::isfinite(ref[0]) || !std::isfinite(ref[1])) return IBO_EHVI_FRONT_BAD_REF;
    std::vector<std::pair<double, double>> p;
    for (int i = 0; i < nfront; i++) {
        const double a = front[2 * (size_t)i], b = front[2 * (size_t)i + 1];
        if (!std::isfinite(a) || !std::isfinite(b)) { if (where) *where = i; return IBO_EHVI_FRONT_BAD_POINT; }
        if (a > ref[0] && b > ref[1]) p.emplace_back(a, b);
    }
    // a descending (b descending among equal a): a point survives when its b exceeds every b seen so far
    std::sort(p.begin(), p.end(), [](const std::pair<double, double> &x, const std::pair<double, double> &y) {
        return x.first > y.first || (x.first == y.first && x.second > y.second);
    });
    std::vector<std::pair<double, double>> keep;
    double best = ref[1];
    for (const auto &q : p)
        if (q.second > best) { keep.push_back(q); best = q.second; }
    if ((long long)keep.size() > max_points) { if (where) *where = (long long)keep.size(); return IBO_EHVI_FRONT_TOO_MANY; }
    out->reserve(2 * keep.size());
    for (size_t i = keep.size(); i-- > 0;) { out->push_back(keep[i].first); out->push_back(keep[i].second); }
    return IBO_EHVI_FRONT_OK;
}
