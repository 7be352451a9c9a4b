// CPU-only checks of the coordinate bisection behind the single-launch CG's blocks (csrc/host_bisect.cpp) on structured squares and cubes:
// rows = grid points in Morton order (the library's internal order), entries = the 6-neighbour (2-D) / 14-neighbour (3-D, Kuhn) stencil,
// cost = entries + 2.  Then the layout builder fed the bisection's numbering (host_build_persist_layout_bisect) on P1 meshes of the library's own
// set-up: its operator application is replayed on the CPU as k_cg_persist runs it and compared with the CSR product of the REAL pattern, which
// is what the mapping of slot_dof and ell_src back to the real numbering has to preserve.
// Prints one "ok" line per case; any failed check ends the program with status 1.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../../fdapde-core_amd/csrc/internal.h"

using namespace fdapde_hip;

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

struct Grid {
    int dim = 0, n = 0;
    int64_t rows = 0;
    std::vector<int32_t> rowptr, col, cost;
    std::vector<uint32_t> q[3];
};

static uint64_t interleave(uint32_t x, uint32_t y, uint32_t z, int dim) {
    uint64_t k = 0;
    for (int b = 0; b < 20; ++b) {
        k |= (uint64_t)((x >> b) & 1u) << (dim * b);
        k |= (uint64_t)((y >> b) & 1u) << (dim * b + 1);
        if (dim == 3) k |= (uint64_t)((z >> b) & 1u) << (dim * b + 2);
    }
    return k;
}

static Grid make_grid(int dim, int n) {
    Grid g;
    g.dim = dim, g.n = n;
    const int nz = dim == 3 ? n : 1;
    g.rows = (int64_t)n * n * nz;
    std::vector<int32_t> order((size_t)g.rows), id((size_t)g.rows);
    std::vector<uint64_t> key((size_t)g.rows);
    auto lin = [&](int x, int y, int z) { return (int32_t)(((int64_t)z * n + y) * n + x); };
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < n; ++y)
            for (int x = 0; x < n; ++x) key[(size_t)lin(x, y, z)] = interleave((uint32_t)x, (uint32_t)y, (uint32_t)z, dim);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key[(size_t)a] < key[(size_t)b]; });
    for (int64_t i = 0; i < g.rows; ++i) id[(size_t)order[(size_t)i]] = (int32_t)i;
    static const int D3[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};
    static const int D2[3][3] = {{1, 0, 0}, {0, 1, 0}, {1, 1, 0}};
    const int nd = dim == 3 ? 7 : 3;
    const double span = (double)(n - 1);   // the lattice itself
    g.rowptr.assign(1, 0);
    for (int a = 0; a < 3; ++a) g.q[a].assign((size_t)g.rows, 0u);
    for (int64_t i = 0; i < g.rows; ++i) {
        const int32_t p = order[(size_t)i];
        const int x = p % n, y = (p / n) % n, z = p / (n * n);
        const int c[3] = {x, y, z};
        for (int a = 0; a < dim; ++a) g.q[a][(size_t)i] = (uint32_t)((double)c[a] / (double)(n - 1) * span + 0.5);
        std::vector<int32_t> cols;
        for (int k = 0; k < nd; ++k)
            for (int s = -1; s <= 1; s += 2) {
                const int* d = dim == 3 ? D3[k] : D2[k];
                const int xx = x + s * d[0], yy = y + s * d[1], zz = z + s * d[2];
                if (xx < 0 || yy < 0 || zz < 0 || xx >= n || yy >= n || zz >= nz) continue;
                cols.push_back(id[(size_t)lin(xx, yy, zz)]);
            }
        std::sort(cols.begin(), cols.end());
        g.col.insert(g.col.end(), cols.begin(), cols.end());
        g.rowptr.push_back((int32_t)g.col.size());
        g.cost.push_back((int32_t)cols.size() + 2);
    }
    return g;
}

static int64_t cross_entries(const Grid& g, const std::vector<int32_t>& block_of) {
    int64_t n = 0;
    for (int64_t i = 0; i < g.rows; ++i)
        for (int32_t k = g.rowptr[(size_t)i]; k < g.rowptr[(size_t)i + 1]; ++k) n += block_of[(size_t)g.col[(size_t)k]] != block_of[(size_t)i];
    return n;
}

// blocks [g0, g0 + g) of the bisection: the left half's cost against its share, at every split down to single blocks
static void check_shares(const std::vector<int64_t>& block_cost, const std::vector<int32_t>& block_rows, int g0, int g, int64_t max_cost) {
    if (g < 2) return;
    const int gl = g / 2;
    int64_t left = 0, total = 0, rows_l = 0, rows_r = 0;
    for (int b = g0; b < g0 + g; ++b) {
        total += block_cost[(size_t)b];
        if (b < g0 + gl) left += block_cost[(size_t)b], rows_l += block_rows[(size_t)b];
        else rows_r += block_rows[(size_t)b];
    }
    const int64_t share = total * gl / g;
    if (rows_l > gl && rows_r > g - gl) CHECK(left >= share && left < share + max_cost);   // (a half held at one row per workgroup is exempt)
    check_shares(block_cost, block_rows, g0, gl, max_cost);
    check_shares(block_cost, block_rows, g0 + gl, g - gl, max_cost);
}

static void run(int dim, int n, int G, bool must_beat_chunks) {
    const Grid g = make_grid(dim, n);
    std::vector<int32_t> perm, rows, perm2, rows2;
    CHECK(host_bisect_partition(g.rows, g.cost.data(), g.q[0].data(), g.q[1].data(), g.q[2].data(), G, perm, rows) == FDAPDE_OK);
    CHECK(host_bisect_partition(g.rows, g.cost.data(), g.q[0].data(), g.q[1].data(), g.q[2].data(), G, perm2, rows2) == FDAPDE_OK);
    CHECK(perm == perm2 && rows == rows2);
    CHECK((int64_t)perm.size() == g.rows && (int)rows.size() == G);
    std::vector<uint8_t> seen((size_t)g.rows, 0);
    for (int32_t r : perm) {
        CHECK(r >= 0 && r < g.rows && !seen[(size_t)r]);
        seen[(size_t)r] = 1;
    }
    int64_t sum = 0;
    for (int32_t r : rows) {
        CHECK(r >= 1);
        sum += r;
    }
    CHECK(sum == g.rows);
    std::vector<int32_t> block_of((size_t)g.rows);
    std::vector<int64_t> block_cost((size_t)G, 0);
    {
        int64_t p = 0;
        for (int b = 0; b < G; ++b)
            for (int32_t k = 0; k < rows[(size_t)b]; ++k, ++p) block_of[(size_t)perm[(size_t)p]] = b, block_cost[(size_t)b] += g.cost[(size_t)perm[(size_t)p]];
    }
    const int64_t max_cost = *std::max_element(g.cost.begin(), g.cost.end());
    check_shares(block_cost, rows, 0, G, max_cost);
    const int64_t cross_b = cross_entries(g, block_of);
    // equal-cost chunks of the internal order: block b starts at the first row whose exclusive cost prefix reaches b * total / G
    const int64_t total = std::accumulate(g.cost.begin(), g.cost.end(), (int64_t)0);
    std::vector<int32_t> chunk_of((size_t)g.rows);
    {
        int64_t cost = 0;
        int b = 0;
        for (int64_t i = 0; i < g.rows; ++i) {
            while (b < G && cost >= (int64_t)b * total / G) ++b;
            chunk_of[(size_t)i] = b - 1;
            cost += g.cost[(size_t)i];
        }
    }
    const int64_t cross_c = cross_entries(g, chunk_of);
    if (must_beat_chunks) CHECK(cross_b < cross_c);
    std::printf("ok %d-D n %d G %d: cross-block entries bisection %lld, chunks %lld (%+.1f %%)\n", dim, n, G, (long long)cross_b, (long long)cross_c,
                100.0 * ((double)cross_b / (double)cross_c - 1.0));
}

// structured P1 mesh of the unit square / cube (Kuhn triangulation), every boundary node a Dirichlet node
static void grid_mesh(int dim, int nx, std::vector<double>& nodes, std::vector<int32_t>& cells, std::vector<uint8_t>& bnd) {
    const int n1 = nx + 1;
    const int64_t nn = dim == 2 ? (int64_t)n1 * n1 : (int64_t)n1 * n1 * n1;
    nodes.assign((size_t)nn * dim, 0.0), bnd.assign((size_t)nn, 0);
    auto id = [&](int i, int j, int k) { return (int32_t)(((int64_t)k * n1 + j) * n1 + i); };
    for (int k = 0; k < (dim == 3 ? n1 : 1); ++k)
        for (int j = 0; j < n1; ++j)
            for (int i = 0; i < n1; ++i) {
                const int32_t p = id(i, j, k);
                nodes[(size_t)p] = (double)i / nx, nodes[(size_t)nn + p] = (double)j / nx;
                if (dim == 3) nodes[(size_t)2 * nn + p] = (double)k / nx;
                bnd[(size_t)p] = i == 0 || j == 0 || i == nx || j == nx || (dim == 3 && (k == 0 || k == nx));
            }
    cells.clear();
    static const int P[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int k = 0; k < (dim == 3 ? nx : 1); ++k)
        for (int j = 0; j < nx; ++j)
            for (int i = 0; i < nx; ++i) {
                if (dim == 2) {
                    const int32_t a = id(i, j, 0), b = id(i + 1, j, 0), c = id(i, j + 1, 0), d = id(i + 1, j + 1, 0);
                    cells.insert(cells.end(), {a, b, d, a, d, c});
                    continue;
                }
                for (const auto& pm : P) {
                    int c[3] = {i, j, k};
                    int32_t v[4];
                    v[0] = id(c[0], c[1], c[2]);
                    for (int s = 0; s < 3; ++s) ++c[pm[s]], v[s + 1] = id(c[0], c[1], c[2]);
                    cells.insert(cells.end(), v, v + 4);
                }
            }
}

static void run_layout(int dim, int nx, int G, bool use_bnd, bool sym) {
    HostSpace hs;
    std::string err;
    std::vector<double> nodes;
    std::vector<int32_t> cells;
    std::vector<uint8_t> bnd;
    grid_mesh(dim, nx, nodes, cells, bnd);
    CHECK(host_set_mesh(hs, dim, dim, (int64_t)bnd.size(), nodes.data(), (int64_t)cells.size() / (dim + 1), cells.data(), bnd.data(), err) == FDAPDE_OK);
    CHECK(host_build_space(hs, 1, err) == FDAPDE_OK);
    std::vector<uint32_t> q;
    host_bisect_quantise(hs.N, hs.n_dofs, hs.dof_coords.data(), hs.dof_i2e.data(), persist_bisect_span(hs.M, hs.N, hs.n_dofs), q);
    PersistLayout pl, chunks;
    std::vector<int32_t> perm, rows;
    CHECK(host_build_persist_layout_bisect(hs, use_bnd, G, 12000, pl, sym ? 1 : 0, q.data(), &perm, &rows) == FDAPDE_OK);
    CHECK(pl.G == G && pl.sym == sym && (int)rows.size() == G);
    const int S = pl.R * kPersistT, nsl = pl.nsl;
    auto dropped = [&](int64_t d) { return use_bnd && hs.dof_bnd_i[(size_t)d]; };
    auto val = [](int64_t row, int64_t col) { return 1.0 + 0.25 * (double)((row + col) % 7); };   // symmetric
    std::vector<double> p((size_t)hs.n_dofs), yref((size_t)hs.n_dofs, 0.0), y((size_t)hs.n_dofs, 0.0);
    for (int64_t d = 0; d < hs.n_dofs; ++d) p[(size_t)d] = dropped(d) ? 0.0 : std::sin(0.37 * (double)d) + 1.5;
    for (int64_t d = 0; d < hs.n_dofs; ++d) {
        if (dropped(d)) continue;
        double acc = p[(size_t)d];
        for (int32_t k = hs.rowptr_i[(size_t)d]; k < hs.rowptr_i[(size_t)d + 1]; ++k) {
            const int32_t c = hs.colidx_i[(size_t)k];
            if (c != d && !dropped(c)) acc += val(d, c) * p[(size_t)c];
        }
        yref[(size_t)d] = acc;
    }
    std::vector<double> board((size_t)pl.n_board, -1e300);
    for (int g = 0; g < pl.G; ++g)
        for (int32_t i = pl.exp_off[(size_t)g]; i < pl.exp_off[(size_t)g + 1]; ++i) {
            const int32_t d = pl.slot_dof[(size_t)g * S + pl.exp_slot[(size_t)i]];
            CHECK(d >= 0);
            board[(size_t)i] = p[(size_t)d];
        }
    std::vector<uint8_t> seen((size_t)hs.n_dofs, 0);
    for (int g = 0; g < pl.G; ++g) {
        const int H = pl.imp_off[(size_t)g + 1] - pl.imp_off[(size_t)g];
        std::vector<double> tab((size_t)(S + H), 0.0);
        int32_t in_block = 0;
        for (int s = 0; s < S; ++s) {
            const int32_t d = pl.slot_dof[(size_t)g * S + s];
            tab[(size_t)s] = d >= 0 ? p[(size_t)d] : 0.0, in_block += d >= 0;
        }
        CHECK(in_block == rows[(size_t)g]);
        for (int h = 0; h < H; ++h) tab[(size_t)(S + h)] = board[(size_t)pl.imp_pos[(size_t)pl.imp_off[(size_t)g] + h]];
        const int32_t* slo = &pl.sl_off[(size_t)g * (nsl + 1)];
        for (int qs = 0; qs < nsl; ++qs)
            for (int l = 0; l < 64; ++l) {
                const int s = qs * 64 + l;
                const int32_t d = pl.slot_dof[(size_t)g * S + s];
                double acc = tab[(size_t)s];
                for (int32_t e = 2 * slo[qs]; e < 2 * slo[qs + 1]; ++e) {
                    const int64_t at = pl.ell_off[(size_t)g] + (int64_t)(e / 2) * 128 + 2 * l + (e & 1);
                    const uint16_t code = pl.ell_code[(size_t)at];
                    const int32_t k = pl.ell_src[(size_t)at];
                    CHECK(code < S + H);
                    if (k < 0) continue;
                    CHECK(d >= 0 && k >= hs.rowptr_i[(size_t)d] && k < hs.rowptr_i[(size_t)d + 1]);   // an entry of the REAL row d
                    const double a = val(d, hs.colidx_i[(size_t)k]);
                    acc += a * tab[code];
                    if (code < S) CHECK(pl.slot_dof[(size_t)g * S + code] == hs.colidx_i[(size_t)k]);
                    if (sym && code < S) y[(size_t)hs.colidx_i[(size_t)k]] += a * tab[(size_t)s];
                }
                if (d >= 0) {
                    CHECK(!seen[(size_t)d]);
                    seen[(size_t)d] = 1, y[(size_t)d] += acc;
                }
            }
    }
    for (int64_t d = 0; d < hs.n_dofs; ++d)
        if (!dropped(d)) CHECK(seen[(size_t)d] && std::fabs(y[(size_t)d] - yref[(size_t)d]) <= 1e-12 * std::fabs(yref[(size_t)d]));
    // the chunk layout of the same system on as many equal blocks, printed next to it: the bisection exchanges fewer vector entries (asserted); its
    // padded entry count may come out either way at these sizes (slice widths), which is why the library compares bytes before it keeps a layout
    std::vector<int32_t> even((size_t)G, (int32_t)(pl.n_int / G));
    even[(size_t)G - 1] += (int32_t)(pl.n_int - (int64_t)G * (pl.n_int / G));
    CHECK(host_build_persist_layout(hs, use_bnd, G, 12000, chunks, even.data(), sym ? 1 : 0) == FDAPDE_OK);
    CHECK(pl.n_board < chunks.n_board);
    std::printf("ok layout %d-D nx %d G %d%s%s: board %lld (chunks %lld), entries %lld (chunks %lld)\n", dim, nx, G, use_bnd ? " dirichlet" : "", sym ? " sym" : "",
                (long long)pl.n_board, (long long)chunks.n_board, (long long)pl.n_entries, (long long)chunks.n_entries);
}

int main() {
    run_layout(3, 20, 9, true, true);
    run_layout(3, 20, 8, false, false);
    run_layout(2, 90, 5, true, true);
    run_layout(2, 64, 12, true, false);
    run(3, 59, 64, true);
    run(3, 80, 256, true);
    run(3, 21, 7, false);
    run(3, 30, 37, false);
    run(2, 200, 16, false);
    run(2, 301, 45, false);
    run(2, 64, 255, false);
    {   // fewer rows than workgroups: refused
        const Grid g = make_grid(2, 3);
        std::vector<int32_t> perm, rows;
        CHECK(host_bisect_partition(g.rows, g.cost.data(), g.q[0].data(), g.q[1].data(), g.q[2].data(), 10, perm, rows) == FDAPDE_EUNSUPPORTED);
    }
    {   // all coordinates equal along two axes (a line in space): still a permutation with no empty block
        const Grid g = make_grid(2, 40);
        std::vector<uint32_t> zero((size_t)g.rows, 0u);
        std::vector<int32_t> perm, rows;
        CHECK(host_bisect_partition(g.rows, g.cost.data(), zero.data(), g.q[1].data(), zero.data(), 13, perm, rows) == FDAPDE_OK);
        std::vector<int32_t> sorted = perm;
        std::sort(sorted.begin(), sorted.end());
        for (int64_t i = 0; i < g.rows; ++i) CHECK(sorted[(size_t)i] == i);
        for (int32_t r : rows) CHECK(r >= 1);
        std::printf("ok degenerate axes\n");
    }
    return 0;
}
