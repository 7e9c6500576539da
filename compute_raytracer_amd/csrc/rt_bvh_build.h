// rt_bvh_build.h -- host side of the bounding-sphere hierarchy (see rt_bvh.hip for the walk and for
// the proof the 4 % radius slack belongs to).  Plain C++17, no HIP: included by rt_bvh.hip, and
// compiled on its own with g++ -fsanitize=address,undefined by tests/test_sanitizers_cpu.py.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

// constants shared with the device side (rt_types.h); repeated here so that the header stands alone
#ifndef RT_FILTER_KAPPA
#define RT_FILTER_KAPPA 1.52587890625e-05f
#define RT_FILTER_EPS 7.62939453125e-06f
#define RT_FILTER_SCALE 1099511627776.0f
#define RT_FILTER_SCALE2 1208925819614629174706176.0f
#endif
#ifndef RT_BVH_SIGMA
#define RT_BVH_SIGMA 1.04   /* node radius = bound of the members x this: the slack of the node test's proof (rt_bvh.hip, header) */
#endif

// ---- host: hierarchy build ---------------------------------------------------------------------------
namespace {

struct Builder {
    const float* rec;              // [n][8] {cx,cy,cz,_, r,g,b, radius}
    std::vector<float>& out_rec;   // 4 floats per node
    std::vector<uint32_t>& out_link;
    std::vector<uint32_t> ids;
    uint32_t arity = 4;            // children per inner node at most (2..8)

    // NaN coordinates order as 0 (a sphere with a NaN in it can never be hit: every comparison of the
    // literal test is false), so that the sorts below keep a strict weak ordering on any input
    double cx(uint32_t i, int a) const {
        const double v = (double)rec[8u * (size_t)i + (size_t)a];
        return v == v ? v : 0.0;
    }
    double rad(uint32_t i) const {
        const double v = std::fabs((double)rec[8u * (size_t)i + 7u]);
        return v == v ? v : 0.0;
    }

    void leaf(uint32_t sphere) {
        out_rec.insert(out_rec.end(), {0.0f, 0.0f, 0.0f, 0.0f});   // filled on the device from geo_f
        out_link.push_back(0x80000000u | sphere);
    }

    // Splits ids[lo,hi) in two.  Up to 32768 members: the position, over all three axes, that
    // minimises  sum over both sides of (squared diagonal of the members' box) * count  -- a
    // surface-area heuristic with the box diagonal as the proxy for the bounding sphere
    // (17 % fewer node tests per ray than the median split on the BASELINE scenes,
    // tools/bvh_sim.py).  Larger ranges: median of the longest axis.  Ties by sphere index.
    uint32_t split2(uint32_t lo, uint32_t hi) {
        const uint32_t n = hi - lo;
        auto by_axis = [&](int ax) {
            return [this, ax](uint32_t a, uint32_t b) {
                const double va = cx(a, ax), vb = cx(b, ax);
                return va < vb || (va == vb && a < b);
            };
        };
        if (n > 32768u) {
            double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (uint32_t k = lo; k < hi; ++k)
                for (int a = 0; a < 3; ++a) {
                    const double v = cx(ids[k], a);
                    mn[a] = std::min(mn[a], v); mx[a] = std::max(mx[a], v);
                }
            int ax = 0;
            if (mx[1] - mn[1] > mx[ax] - mn[ax]) ax = 1;
            if (mx[2] - mn[2] > mx[ax] - mn[ax]) ax = 2;
            const uint32_t mid = lo + n / 2u;
            std::nth_element(ids.begin() + lo, ids.begin() + mid, ids.begin() + hi, by_axis(ax));
            return mid;
        }
        double best = INFINITY;
        int best_ax = 0;
        uint32_t best_k = n / 2u;
        std::vector<uint32_t> order(n);
        std::vector<double> suffix(n);
        for (int ax = 0; ax < 3; ++ax) {
            std::copy(ids.begin() + lo, ids.begin() + hi, order.begin());
            std::sort(order.begin(), order.end(), by_axis(ax));
            double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
            auto grow = [&](uint32_t i) {
                double d2 = 0.0;
                for (int a = 0; a < 3; ++a) {
                    mn[a] = std::min(mn[a], cx(i, a) - rad(i));
                    mx[a] = std::max(mx[a], cx(i, a) + rad(i));
                    d2 += (mx[a] - mn[a]) * (mx[a] - mn[a]);
                }
                return d2;
            };
            for (uint32_t k = n; k-- > 1u;) suffix[k] = grow(order[k]) * (double)(n - k);   // members k..n-1
            for (int a = 0; a < 3; ++a) { mn[a] = INFINITY; mx[a] = -INFINITY; }
            for (uint32_t k = 1; k < n; ++k) {                                              // members 0..k-1 | k..n-1
                const double cost = grow(order[k - 1u]) * (double)k + suffix[k];
                if (cost < best) { best = cost; best_ax = ax; best_k = k; }
            }
        }
        std::sort(ids.begin() + lo, ids.begin() + hi, by_axis(best_ax));
        return lo + best_k;
    }

    // bounding sphere of ids[lo,hi): centre of the members' box, then shrink-wrapped -- the centre
    // moves towards the farthest member while that reduces the radius
    // sphere (optional): the centre as stored and the radius about it WITHOUT sigma, in f64, for the optimiser's cost
    void bound(uint32_t lo, uint32_t hi, float out[4], double* sphere = nullptr) {
        double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t k = lo; k < hi; ++k)
            for (int a = 0; a < 3; ++a) {
                mn[a] = std::min(mn[a], cx(ids[k], a) - rad(ids[k]));
                mx[a] = std::max(mx[a], cx(ids[k], a) + rad(ids[k]));
            }
        auto radius_at = [&](const double P[3], uint32_t& far) {
            double R = -1.0;
            for (uint32_t k = lo; k < hi; ++k) {
                const uint32_t i = ids[k];
                const double dx = cx(i, 0) - P[0], dy = cx(i, 1) - P[1], dz = cx(i, 2) - P[2];
                const double d = std::sqrt(dx * dx + dy * dy + dz * dz) + rad(i);
                if (d > R) { R = d; far = i; }
            }
            return R;
        };
        double P[3] = {0.5 * (mn[0] + mx[0]), 0.5 * (mn[1] + mx[1]), 0.5 * (mn[2] + mx[2])};
        uint32_t far = ids[lo];
        double Rp = radius_at(P, far);
        for (int it = 0; it < 32; ++it) {
            const double s[3] = {cx(far, 0) - P[0], cx(far, 1) - P[1], cx(far, 2) - P[2]};
            const double len = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
            if (!(len > 1e-12)) break;
            const double Q[3] = {P[0] + s[0] / len * 0.05 * Rp, P[1] + s[1] / len * 0.05 * Rp, P[2] + s[2] / len * 0.05 * Rp};
            uint32_t far_q = far;
            const double Rq = radius_at(Q, far_q);
            if (!(Rq < Rp)) break;
            P[0] = Q[0]; P[1] = Q[1]; P[2] = Q[2]; Rp = Rq; far = far_q;
        }
        // ... then towards the farthest member with a shrinking step (Badoiu-Clarkson: converges on the smallest enclosing
        // ball; the greedy walk above stops at its first non-improvement, typically 2 % in radius short of it), keeping
        // the best centre seen.  Any centre is valid -- the radius is measured afterwards --, a smaller ball is passed by fewer rays.
        if (hi - lo > 2u) {
            double Q[3] = {P[0], P[1], P[2]};
            for (int it = 1; it <= 96; ++it) {
                uint32_t fq = far;
                const double Rq = radius_at(Q, fq);
                if (Rq < Rp) { Rp = Rq; P[0] = Q[0]; P[1] = Q[1]; P[2] = Q[2]; }
                const double s[3] = {cx(fq, 0) - Q[0], cx(fq, 1) - Q[1], cx(fq, 2) - Q[2]};
                const double len = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
                if (!(len > 1e-12)) break;
                // the farthest POINT of the farthest member: its centre pushed out by its radius
                const double k = (1.0 + rad(fq) / len) / (double)(it + 1);
                Q[0] += s[0] * k; Q[1] += s[1] * k; Q[2] += s[2] * k;
            }
        }
        const float C[3] = {(float)P[0], (float)P[1], (float)P[2]};   // the record stores the centre in fp32:
        const double Cd[3] = {C[0], C[1], C[2]};                       // the radius is taken about THAT point
        uint32_t unused = 0;
        double R = radius_at(Cd, unused);
        if (sphere) { sphere[0] = Cd[0]; sphere[1] = Cd[1]; sphere[2] = Cd[2]; sphere[3] = R; }
        R *= RT_BVH_SIGMA;            // sigma, see the header
        const double c2 = (double)C[0] * C[0] + (double)C[1] * C[1] + (double)C[2] * C[2];
        const double k = c2 * (1.0 - (double)RT_FILTER_EPS) - R * R * (1.0 + (double)RT_FILTER_KAPPA);
        out[0] = C[0] * RT_FILTER_SCALE; out[1] = C[1] * RT_FILTER_SCALE; out[2] = C[2] * RT_FILTER_SCALE;
        out[3] = (float)(k * (double)RT_FILTER_SCALE2);
    }

    // ---- the tree as an explicit structure: built top-down, optimised (below), then emitted threaded ----
    static constexpr uint32_t ROOT = 0xFFFFFFFFu;   // parent of the top-level nodes (there is no root node: `top` lists them)
    struct Node {
        uint32_t parent = ROOT, nk = 0, sphere = 0;   // nk == 0: a leaf (or a node the optimiser dissolved: dead)
        uint32_t kid[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        double s[4] = {0.0, 0.0, 0.0, 0.0};           // a ball that bounds the members: centre, radius without sigma
        float rec[4] = {0.0f, 0.0f, 0.0f, 0.0f};      // bound() of the members, and its radius (without sigma): what the
        double r_rec = 0.0;                           // walk will read, and what the tree's cost is counted with
        bool dirty = false;                           // the SET of members changed since: bound() again at emission
        bool fixed = false;                           // a top-level large-sphere leaf: stays where it is
        bool dead = false;
    };
    std::vector<Node> nodes;
    std::vector<uint32_t> top;

    uint32_t new_leaf(uint32_t sphere, uint32_t parent) {
        Node l;
        l.parent = parent; l.sphere = sphere;
        l.s[0] = cx(sphere, 0); l.s[1] = cx(sphere, 1); l.s[2] = cx(sphere, 2); l.s[3] = rad(sphere);
        nodes.push_back(l);
        return (uint32_t)nodes.size() - 1u;
    }
    void add_kid(uint32_t parent, uint32_t k) {
        if (parent == ROOT) top.push_back(k); else nodes[parent].kid[nodes[parent].nk++] = k;
    }

    uint32_t make(uint32_t lo, uint32_t hi, uint32_t parent) {
        if (hi - lo == 1u) return new_leaf(ids[lo], parent);
        const uint32_t me = (uint32_t)nodes.size();
        nodes.emplace_back();
        nodes[me].parent = parent;
        children(lo, hi, me);
        float b[4];
        double s[4];
        bound(lo, hi, b, s);
        std::copy(b, b + 4, nodes[me].rec);
        std::copy(s, s + 4, nodes[me].s);
        nodes[me].r_rec = s[3];
        return me;
    }

    // up to `arity` children (four: C3 1.50 / 1.55 / 1.61 / 1.65 ms with 4 / 5 / 6 / 8, profiles/r04/bvh_arity_probe.log): the largest
    // part BY MEMBER COUNT is split until there are that many.  Choosing the part by cost (count x squared diagonal) or by
    // radius instead is no better -- C3, simulated tests per ray: 47.5 by count, 47.6 by cost, 47.8 by radius; exact-radius
    // splits 49.1 / 48.6, binary splits collapsed to four 47.8 (docs/experiments.md) --, so this stays; what the top-down
    // pass leaves on the table is taken by optimise() below.
    void children(uint32_t lo, uint32_t hi, uint32_t parent) {
        if (hi - lo <= arity) {
            for (uint32_t k = lo; k < hi; ++k) add_kid(parent, new_leaf(ids[k], parent));
            return;
        }
        uint32_t cut[9] = {lo, hi, 0, 0, 0, 0, 0, 0, 0};     // sorted part boundaries
        int parts = 1;
        while (parts < (int)arity) {
            int big = 0;
            for (int j = 1; j < parts; ++j)
                if (cut[j + 1] - cut[j] > cut[big + 1] - cut[big]) big = j;
            if (cut[big + 1] - cut[big] < 2u) break;
            const uint32_t mid = split2(cut[big], cut[big + 1]);
            for (int j = parts; j > big; --j) cut[j + 1] = cut[j];
            cut[big + 1] = mid;
            ++parts;
        }
        for (int j = 0; j < parts; ++j) {
            const uint32_t k = make(cut[j], cut[j + 1], parent);
            add_kid(parent, k);
        }
    }

    // ---- emission: depth-first, skip links as 4 * index.  `ids` is refilled in the order of emission, so that a node's
    // members are ids[first, last) again whatever the optimiser did to the grouping.  Returns the tree's cost. ----
    static double ball_cost(const Node& x) { return x.nk ? x.s[3] * x.s[3] * (double)x.nk : 0.0; }       // the optimiser's working balls
    static double rec_cost(const Node& x) { return x.nk ? x.r_rec * x.r_rec * (double)x.nk : 0.0; }     // the records' radii
    void emit(uint32_t node, double& cost) {
        if (nodes[node].nk == 0u) { ids.push_back(nodes[node].sphere); leaf(nodes[node].sphere); return; }
        const size_t me = out_link.size();
        const uint32_t first = (uint32_t)ids.size();
        out_rec.insert(out_rec.end(), {0.0f, 0.0f, 0.0f, 0.0f});
        out_link.push_back(0u);
        for (uint32_t k = 0; k < nodes[node].nk; ++k) emit(nodes[node].kid[k], cost);
        if (nodes[node].dirty) {
            bound(first, (uint32_t)ids.size(), nodes[node].rec, nodes[node].s);
            nodes[node].r_rec = nodes[node].s[3];
            nodes[node].dirty = false;
        }
        cost += rec_cost(nodes[node]);
        std::copy(nodes[node].rec, nodes[node].rec + 4, out_rec.begin() + 4 * me);
        out_link[me] = 4u * (uint32_t)out_link.size();  // skip link: first node after this subtree, as 4 * index
    }
    double emit_all() {
        out_rec.clear(); out_link.clear(); ids.clear();
        double cost = 0.0;
        for (uint32_t t : top) emit(t, cost);
        return cost;
    }

    // ---- optimisation by reinsertion (Bittner, Hapala, Havran 2013, "Fast insertion-based optimization of bounding
    // volume hierarchies", adapted to bounding spheres, up to `arity` children and a threaded layout) ----
    // A ray that passes a node tests all its children, and the chance that a line through the scene passes a ball goes
    // with its cross section:  cost = sum over inner nodes of R^2 x children.  A pass takes subtrees (single leaves
    // included) out of their parents, most expensive parents first (the costlier half of them), and puts it back where the cost rises least, found by a
    // branch-and-bound descent from the top; a move is kept only if the cost of the nodes it touched fell, otherwise
    // every node is restored.  A parent left with one child is replaced by that child; a subtree joins a node with a free
    // slot, or -- exactly when its old parent was dissolved -- is paired with a node under a new one, so that the node count
    // stays the top-down build's (the kernel form of a scene follows its node count: rt_bvh.hip launch_bvh).  Balls on the two paths are refitted
    // from the children's balls (never larger than what they replace where members only left); the records the walk reads
    // come from bound() over the members at emission, and rt_bvh_build keeps the top-down tree if those say the cost rose.
    // Deterministic: no clock, no random numbers; ties by node index.
    std::vector<std::pair<uint32_t, Node>> journal;       // nodes as they were before the move in progress
    std::vector<std::pair<uint32_t, uint32_t>> top_journal;
    std::vector<uint32_t> stamp;
    std::vector<std::pair<double, uint32_t>> search_heap;
    uint32_t txn = 0, inner_live = 0;          // txn: one per move tried or kept, far fewer than 2^32 (passes x nodes, n <= 32,768)

    void touch(uint32_t i) {
        if (stamp.size() < nodes.size()) stamp.resize(nodes.size(), 0u);
        if (stamp[i] == txn) return;
        stamp[i] = txn;
        journal.emplace_back(i, nodes[i]);
    }
    static void merge2(const double a[4], const double b[4], double o[4]) {
        const double d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
        const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (len + b[3] <= a[3]) { const double t[4] = {a[0], a[1], a[2], a[3]}; std::copy(t, t + 4, o); return; }
        if (len + a[3] <= b[3]) { const double t[4] = {b[0], b[1], b[2], b[3]}; std::copy(t, t + 4, o); return; }
        const double R = 0.5 * (len + a[3] + b[3]);
        const double f = len > 0.0 ? (R - a[3]) / len : 0.0;
        const double t[4] = {a[0] + d[0] * f, a[1] + d[1] * f, a[2] + d[2] * f, R};
        std::copy(t, t + 4, o);
    }
    // ball of the children's balls: merged one by one, then a few steps towards the farthest child, best centre kept
    void kids_ball(const Node& x, double o[4]) const {
        std::copy(nodes[x.kid[0]].s, nodes[x.kid[0]].s + 4, o);
        for (uint32_t k = 1; k < x.nk; ++k) merge2(o, nodes[x.kid[k]].s, o);
        if (x.nk < 3u) return;
        double q[3] = {o[0], o[1], o[2]};
        for (int it = 1; it <= 8; ++it) {
            double R = -1.0, len_f = 0.0;
            uint32_t far = 0;
            for (uint32_t k = 0; k < x.nk; ++k) {
                const double* c = nodes[x.kid[k]].s;
                const double len = std::sqrt((c[0] - q[0]) * (c[0] - q[0]) + (c[1] - q[1]) * (c[1] - q[1]) + (c[2] - q[2]) * (c[2] - q[2]));
                if (len + c[3] > R) { R = len + c[3]; far = k; len_f = len; }
            }
            if (R < o[3]) { o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = R; }
            if (!(len_f > 1e-300)) break;
            const double* c = nodes[x.kid[far]].s;
            const double f = (1.0 + c[3] / len_f) / (double)(it + 1);
            q[0] += (c[0] - q[0]) * f; q[1] += (c[1] - q[1]) * f; q[2] += (c[2] - q[2]) * f;
        }
    }
    // refits x and its ancestors after a subtree with ball `added` joined below (nullptr: after one left)
    void refit_up(uint32_t x, const double* added) {
        for (; x != ROOT; x = nodes[x].parent) {
            double alt[4], nb[4];
            if (added) merge2(nodes[x].s, added, alt); else std::copy(nodes[x].s, nodes[x].s + 4, alt);
            kids_ball(nodes[x], nb);
            const double* pick = nb[3] < alt[3] ? nb : alt;
            if (pick[0] == nodes[x].s[0] && pick[1] == nodes[x].s[1] && pick[2] == nodes[x].s[2] && pick[3] == nodes[x].s[3]) {
                if (!added) break;             // nothing above changes either (a ball that grew may still stick out further up)
                continue;
            }
            touch(x);
            std::copy(pick, pick + 4, nodes[x].s);
        }
    }
    void replace_kid(uint32_t parent, uint32_t was, uint32_t now) {
        if (parent == ROOT) {
            for (uint32_t k = 0; k < (uint32_t)top.size(); ++k)
                if (top[k] == was) { top_journal.emplace_back(k, was); top[k] = now; return; }
            return;
        }
        touch(parent);
        for (uint32_t k = 0; k < nodes[parent].nk; ++k)
            if (nodes[parent].kid[k] == was) { nodes[parent].kid[k] = now; return; }
    }
    void detach(uint32_t s) {
        const uint32_t p = nodes[s].parent;
        touch(p); touch(s);
        Node& P = nodes[p];
        uint32_t w = 0;
        for (uint32_t k = 0; k < P.nk; ++k) if (P.kid[k] != s) P.kid[w++] = P.kid[k];
        P.nk = w;
        nodes[s].parent = ROOT;
        uint32_t from = p;
        if (P.nk == 1u) {                      // one child left: it takes the node's place
            const uint32_t q = P.kid[0], g = P.parent;
            touch(q);
            nodes[q].parent = g;
            replace_kid(g, p, q);
            nodes[p].nk = 0; nodes[p].dead = true;
            --inner_live;
            from = g;
        }
        refit_up(from, nullptr);
    }
    // where the cost rises least: (node, pair) -- pair: under a new node with it, else as one more child of it
    bool find_place(uint32_t s, bool allow_pair, bool allow_child, uint32_t& where, bool& pair) {
        typedef std::pair<double, uint32_t> Item;     // (cost induced on the ancestors, node)
        auto later = [](const Item& a, const Item& b) { return a.first > b.first || (a.first == b.first && a.second > b.second); };
        std::vector<Item>& heap = search_heap;
        heap.clear();
        for (uint32_t t : top)
            if (!nodes[t].fixed) { heap.emplace_back(0.0, t); std::push_heap(heap.begin(), heap.end(), later); }
        double best = INFINITY;
        bool found = false;
        const double* S = nodes[s].s;
        int budget = 256;                              // nodes examined per search: bounded work
        while (!heap.empty() && budget-- > 0) {
            std::pop_heap(heap.begin(), heap.end(), later);
            const Item it = heap.back();
            heap.pop_back();
            if (!(it.first < best)) break;
            const Node& X = nodes[it.second];
            double m[4];
            merge2(X.s, S, m);
            const double m2 = m[3] * m[3];
            if (allow_pair) {
                const double c = it.first + 2.0 * m2;
                if (c < best) { best = c; where = it.second; pair = true; found = true; }
            }
            if (X.nk) {
                const double down = it.first + (m2 - X.s[3] * X.s[3]) * (double)X.nk;
                if (allow_child && X.nk < arity && down + m2 < best) { best = down + m2; where = it.second; pair = false; found = true; }
                if (down < best)
                    for (uint32_t k = 0; k < X.nk; ++k) { heap.emplace_back(down, X.kid[k]); std::push_heap(heap.begin(), heap.end(), later); }
            }
        }
        return found;
    }
    void attach(uint32_t s, uint32_t where, bool pair) {
        double S[4];
        std::copy(nodes[s].s, nodes[s].s + 4, S);
        touch(s);
        if (!pair) {
            touch(where);
            nodes[where].kid[nodes[where].nk++] = s;
            nodes[s].parent = where;
            refit_up(where, S);
            return;
        }
        const uint32_t g = nodes[where].parent;
        const uint32_t nn = (uint32_t)nodes.size();
        nodes.emplace_back();
        Node& N = nodes[nn];
        N.parent = g; N.nk = 2; N.kid[0] = where; N.kid[1] = s; N.dirty = true;
        merge2(nodes[where].s, S, N.s);
        replace_kid(g, where, nn);
        touch(where);
        nodes[where].parent = nn;
        nodes[s].parent = nn;
        ++inner_live;
        refit_up(g, S);
    }
    // after a move from under `from` to under `to`: the nodes whose SET of members changed are those on the two paths below
    // their lowest common ancestor; from there up the members are the same and the bound the top-down build took stands
    // (the big nodes near the top, whose bound() costs most, are rarely touched: most moves are local)
    void mark_dirty(uint32_t from, uint32_t to) {
        ++txn;
        if (stamp.size() < nodes.size()) stamp.resize(nodes.size(), 0u);
        for (uint32_t x = to; x != ROOT; x = nodes[x].parent) stamp[x] = txn;
        uint32_t lca = from;
        while (lca != ROOT && stamp[lca] != txn) { nodes[lca].dirty = true; lca = nodes[lca].parent; }
        for (uint32_t x = to; x != lca; x = nodes[x].parent) nodes[x].dirty = true;
    }
    // returns the number of moves kept
    uint32_t optimise(uint32_t passes) {
        uint32_t inner_topdown = 0;
        for (const Node& x : nodes) inner_topdown += x.nk ? 1u : 0u;
        inner_live = inner_topdown;
        uint32_t moves = 0;
        std::vector<std::pair<double, uint32_t>> cand;
        for (uint32_t pass = 0; pass < passes; ++pass) {
            cand.clear();
            for (uint32_t i = 0; i < (uint32_t)nodes.size(); ++i) {
                const Node& x = nodes[i];
                if (x.dead || x.parent == ROOT) continue;
                const double r = nodes[x.parent].s[3];
                cand.emplace_back(r == r ? r : 0.0, i);
            }
            std::sort(cand.begin(), cand.end(), [](const std::pair<double, uint32_t>& a, const std::pair<double, uint32_t>& b) {
                return a.first > b.first || (a.first == b.first && a.second < b.second);
            });
            // Bounded work, and a bound on what the build may cost on the frame path (a count change builds inline): the costlier
            // half of the parents only.  A try costs about 2 us whatever comes of it, the whole top-down build about 5 us a sphere;
            // all candidates in two passes made the build 3.3 x as long for a cost 4.0 % lower (C3), this half in one pass
            // 1.6-1.9 x for 2.2 % (docs/experiments.md).
            const size_t tries = (cand.size() + 1u) / 2u;
            uint32_t kept = 0;
            for (size_t ci = 0; ci < tries; ++ci) {
                const auto& cd = cand[ci];
                const uint32_t s = cd.second;
                if (nodes[s].dead || nodes[s].parent == ROOT) continue;
                uint32_t depth = 0;
                for (uint32_t a = nodes[s].parent; a != ROOT && depth <= 64u; a = nodes[a].parent) ++depth;
                if (depth > 64u) continue;                                 // bounded work on degenerate (chain-like) trees
                ++txn;
                journal.clear(); top_journal.clear();
                const size_t size0 = nodes.size();
                const uint32_t live0 = inner_live, old_parent = nodes[s].parent;
                detach(s);
                uint32_t where = 0;
                bool pair = false;
                // the node count stays EXACTLY the top-down tree's (which kernel form a scene gets follows it, and scenes are
                // placed on either side of a form's edge by it): a move that dissolved the parent pairs the subtree with a node
                // under a new one, any other move takes a free slot
                const bool dissolved = inner_live < live0;
                bool ok = find_place(s, dissolved, !dissolved, where, pair);
                if (ok && !pair && where == old_parent && !nodes[old_parent].dead) ok = false;   // back where it was
                double delta = 0.0;
                if (ok) {
                    attach(s, where, pair);
                    for (const auto& j : journal) delta += ball_cost(nodes[j.first]) - ball_cost(j.second);
                    for (size_t i = size0; i < nodes.size(); ++i) delta += ball_cost(nodes[i]);
                }
                if (ok && delta < 0.0) {
                    mark_dirty(old_parent, nodes[s].parent);          // (a dissolved parent still knows its own)
                    ++moves; ++kept;
                } else {
                    nodes.resize(size0);
                    for (size_t i = journal.size(); i-- > 0;) nodes[journal[i].first] = journal[i].second;
                    for (size_t i = top_journal.size(); i-- > 0;) top[top_journal[i].first] = top_journal[i].second;
                    inner_live = live0;
                }
            }
            if (!kept) break;
        }
        return moves;
    }
};

}  // namespace

// reinsertion passes over the top-down tree (Builder::optimise); 0: the top-down tree as built.  The library takes the
// number from its public header, a stand-alone build of this file from here.
#ifndef RT_BVH_OPT_PASSES
#ifdef RT355_HIERARCHY_PASSES
#define RT_BVH_OPT_PASSES RT355_HIERARCHY_PASSES
#else
#define RT_BVH_OPT_PASSES 1u
#endif
#endif

struct rt_bvh_build_info {
    uint32_t nodes_topdown = 0;          // node count of the top-down tree (the optimised one has the same)
    uint32_t moves = 0;                  // reinsertions kept
    double cost_topdown = 0.0, cost = 0.0;   // sum over inner nodes of (radius without sigma)^2 x children, from the emitted bounds
};

// Builds the threaded hierarchy.  Top level: spheres much larger than the scene (a ground
// sphere) as leaves of their own -- inside a node they would inflate it to cover everything --,
// then up to four subtrees over the rest, built top-down and then optimised by reinsertion (not above 32,768 spheres,
// the range of the median split).  Returns the node count n; the arrays hold n + 1
// entries, the last one being the sentinel the traversal loop parks finished lanes on.
inline uint32_t rt_bvh_build(const float* records, uint32_t n, std::vector<float>& rec4, std::vector<uint32_t>& link, uint32_t arity = 4u,
                             uint32_t passes = RT_BVH_OPT_PASSES, rt_bvh_build_info* info = nullptr) {
    rec4.clear(); link.clear();
    if (info) *info = rt_bvh_build_info();
    if (n == 0) return 0;
    rec4.reserve((size_t)n * 6u); link.reserve((size_t)n * 3u / 2u + 8u);
    Builder b{records, rec4, link, {}};
    b.arity = arity < 2u ? 2u : (arity > 8u ? 8u : arity);
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], b.cx(i, a)); mx[a] = std::max(mx[a], b.cx(i, a)); }
    // median radius: a sphere is "large" when it exceeds 8 medians AND an eighth of the centres' extent
    std::vector<double> radii(n);
    for (uint32_t i = 0; i < n; ++i) radii[i] = b.rad(i);
    std::nth_element(radii.begin(), radii.begin() + n / 2u, radii.end());
    const double med = radii[n / 2u];
    const double ext = std::sqrt((mx[0] - mn[0]) * (mx[0] - mn[0]) + (mx[1] - mn[1]) * (mx[1] - mn[1]) + (mx[2] - mn[2]) * (mx[2] - mn[2]));
    b.nodes.reserve((size_t)n * 2u + 8u);
    uint32_t big = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const bool large = n > 8u && b.rad(i) > 8.0 * med && b.rad(i) > 0.125 * ext;
        if (large && big < 64u) {
            const uint32_t l = b.new_leaf(i, Builder::ROOT);
            b.nodes[l].fixed = true;
            b.top.push_back(l);
            ++big;
        } else b.ids.push_back(i);
    }
    const uint32_t rest = (uint32_t)b.ids.size();
    if (rest) b.children(0u, rest, Builder::ROOT);
    double cost0 = 0.0;
    bool finite = true;
    for (const Builder::Node& x : b.nodes) {
        cost0 += Builder::rec_cost(x);
        finite = finite && std::isfinite(x.s[0]) && std::isfinite(x.s[1]) && std::isfinite(x.s[2]) && std::isfinite(x.s[3]);
    }
    const uint32_t nodes_topdown = (uint32_t)b.nodes.size();
    uint32_t moves = 0;
    double cost = cost0;
    if (passes && rest <= 32768u && finite && std::isfinite(cost0)) {
        const std::vector<Builder::Node> nodes0 = b.nodes;      // the top-down tree, should the optimised one not be better
        const std::vector<uint32_t> top0 = b.top;
        moves = b.optimise(passes);
        if (moves) {
            cost = b.emit_all();
            if (!(cost <= cost0) || link.size() > nodes0.size()) {
                b.nodes = nodes0; b.top = top0;
                moves = 0;
                cost = b.emit_all();
            }
        } else cost = b.emit_all();
    } else cost = b.emit_all();
    const uint32_t nodes = (uint32_t)link.size();
    if (info) {
        info->nodes_topdown = nodes_topdown;
        info->moves = moves; info->cost_topdown = cost0; info->cost = cost;
    }
    rec4.insert(rec4.end(), {0.0f, 0.0f, 0.0f, INFINITY});   // sentinel [nodes]: never passes, links to itself
    link.push_back(4u * nodes);
    return nodes;
}
