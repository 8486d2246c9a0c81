// Stand-alone host check of the mesh ray casting (youreditableavatar_amd/csrc/tgs_mesh_rays.hpp): builds the tree of a few meshes, casts rays in both
// modes and compares bits, checks the occlusion query against the cast, the hit-face array against the returned faces, exact ties on the cube,
// invalid rays, and a tree with a corrupt header or corrupt words.  Host code only, with its own main: it is not loaded into Python and needs no
// device.  Meant to be built with the host sanitizers:
//
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/mesh_rays_host_check.cpp -o mesh_rays_host_check
//     ./mesh_rays_host_check           (prints one line per mesh; exit status 0 when everything holds)
#include "../youreditableavatar_amd/csrc/tgs_mesh_rays.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

using namespace tgs::msdf;
namespace mr = tgs::mrays;

struct Mesh { std::vector<float> v; std::vector<int32_t> f; };

static Mesh cube()                                                                  // [0,1]^3, the -z side first: faces 0 and 1 share the diagonal x == y
{
    Mesh m;
    for (int i = 0; i < 8; ++i) { m.v.push_back((i & 1) ? 1.0f : 0.0f); m.v.push_back((i & 2) ? 1.0f : 0.0f); m.v.push_back((i & 4) ? 1.0f : 0.0f); }
    const int q[6][4] = {{0, 2, 3, 1}, {0, 1, 5, 4}, {2, 6, 7, 3}, {0, 4, 6, 2}, {1, 3, 7, 5}, {4, 5, 7, 6}};
    for (auto& s : q) { const int t[6] = {s[0], s[1], s[2], s[0], s[2], s[3]}; m.f.insert(m.f.end(), t, t + 6); }
    return m;
}

static Mesh icosphere(int levels)
{
    Mesh m;
    const float t = 1.6180339887f;
    const float v[12][3] = {{-1, t, 0}, {1, t, 0}, {-1, -t, 0}, {1, -t, 0}, {0, -1, t}, {0, 1, t}, {0, -1, -t}, {0, 1, -t}, {t, 0, -1}, {t, 0, 1}, {-t, 0, -1}, {-t, 0, 1}};
    const int f[20][3] = {{0, 11, 5}, {0, 5, 1}, {0, 1, 7}, {0, 7, 10}, {0, 10, 11}, {1, 5, 9}, {5, 11, 4}, {11, 10, 2}, {10, 7, 6}, {7, 1, 8},
                          {3, 9, 4}, {3, 4, 2}, {3, 2, 6}, {3, 6, 8}, {3, 8, 9}, {4, 9, 5}, {2, 4, 11}, {6, 2, 10}, {8, 6, 7}, {9, 8, 1}};
    auto push = [&m](float x, float y, float z) { const float n = sqrtf(x * x + y * y + z * z); m.v.push_back(x / n); m.v.push_back(y / n); m.v.push_back(z / n); return (int)(m.v.size() / 3 - 1); };
    for (auto& p : v) push(p[0], p[1], p[2]);
    for (auto& p : f) m.f.insert(m.f.end(), p, p + 3);
    for (int l = 0; l < levels; ++l) {
        std::map<std::pair<int, int>, int> mid;
        std::vector<int32_t> nf;
        auto middle = [&](int a, int b) {
            const std::pair<int, int> key(a < b ? a : b, a < b ? b : a);
            auto it = mid.find(key);
            if (it != mid.end()) return it->second;
            const int k = push(m.v[3 * a] + m.v[3 * b], m.v[3 * a + 1] + m.v[3 * b + 1], m.v[3 * a + 2] + m.v[3 * b + 2]);
            mid[key] = k;
            return k;
        };
        for (size_t k = 0; k < m.f.size(); k += 3) {
            const int a = m.f[k], b = m.f[k + 1], c = m.f[k + 2], ab = middle(a, b), bc = middle(b, c), ca = middle(c, a);
            const int t4[12] = {a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca};
            nf.insert(nf.end(), t4, t4 + 12);
        }
        m.f.swap(nf);
    }
    return m;
}

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s; }
static float unit(uint32_t& s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f); }      // [0, 1)

struct Out {
    std::vector<float> t, uv, normal;
    std::vector<int32_t> face, geom;
    std::vector<uint8_t> hit;                                                       // F bytes between two guard bands of 64
    explicit Out(long long N, int F) : t((size_t)N, 7.0f), uv(2 * (size_t)N, 7.0f), normal(3 * (size_t)N, 7.0f), face((size_t)N, 7), geom((size_t)N, 7), hit((size_t)F + 128, 0) {}
    bool same(const Out& o) const
    {
        return memcmp(t.data(), o.t.data(), sizeof(float) * t.size()) == 0 && memcmp(uv.data(), o.uv.data(), sizeof(float) * uv.size()) == 0 &&
               memcmp(normal.data(), o.normal.data(), sizeof(float) * normal.size()) == 0 && face == o.face && geom == o.geom && hit == o.hit;
    }
    bool bands_clear(int F) const
    {
        for (int k = 0; k < 64; ++k) if (hit[(size_t)k] || hit[(size_t)F + 64 + (size_t)k]) return false;
        return true;
    }
};

static const char* cast(const std::vector<char>& tree, const Mesh& m, const std::vector<float>& rays, int mode, Out& o)
{
    const int V = (int)(m.v.size() / 3), F = (int)(m.f.size() / 3);
    return mr::cast_host(tree.data(), tree.size(), V, F, m.v.data(), m.f.data(), 0, (long long)(rays.size() / 6), rays.data(), mode, o.t.data(), o.face.data(), o.geom.data(), o.uv.data(),
                         o.normal.data(), o.hit.data() + 64);
}

static void push_ray(std::vector<float>& rays, float ox, float oy, float oz, float dx, float dy, float dz)
{
    const float r[6] = {ox, oy, oz, dx, dy, dz};
    rays.insert(rays.end(), r, r + 6);
}

static void check(const char* name, const Mesh& m, int n_rays)
{
    const int V = (int)(m.v.size() / 3), F = (int)(m.f.size() / 3);
    std::vector<char> tree(tree_bytes((size_t)F), (char)0x5a);
    CHECK(build_tree(V, F, m.v.data(), m.f.data(), 0, tree.data(), tree.size()) == nullptr);
    const Header* h = (const Header*)tree.data();

    std::vector<float> rays;
    uint32_t s = 2024u;
    for (int k = 0; k < n_rays; ++k) {                                               // origins within [-6, 6]^3, aimed at points of [-1, 1]^3
        const float o[3] = {12.0f * unit(s) - 6.0f, 12.0f * unit(s) - 6.0f, 12.0f * unit(s) - 6.0f};
        const float scale = 0.25f + 2.0f * unit(s);
        push_ray(rays, o[0], o[1], o[2], (2.0f * unit(s) - 1.0f - o[0]) * scale, (2.0f * unit(s) - 1.0f - o[1]) * scale, (2.0f * unit(s) - 1.0f - o[2]) * scale);
    }
    for (int k = 0; k < 8 && k < V; ++k) push_ray(rays, 3.0f, -2.5f, 4.0f, m.v[3 * (size_t)k] - 3.0f, m.v[3 * (size_t)k + 1] + 2.5f, m.v[3 * (size_t)k + 2] - 4.0f);      // through vertices
    for (float p : {-0.5f, 0.0f, 0.25f, 0.5f, 1.0f}) for (float q : {-0.5f, 0.0f, 0.5f, 1.0f}) {                          // a dyadic grid of axis rays: exact ties on the cube
        push_ray(rays, p, q, -2.0f, 0.0f, 0.0f, 1.0f); push_ray(rays, -2.0f, p, q, 2.0f, 0.0f, 0.0f); push_ray(rays, q, 3.0f, p, 0.0f, -0.5f, 0.0f);
    }
    const long long valid = (long long)(rays.size() / 6);
    push_ray(rays, NAN, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f);
    push_ray(rays, 0.5f, 0.5f, -2.0f, 0.0f, INFINITY, 1.0f);
    push_ray(rays, 0.5f, 0.5f, -2.0f, 0.0f, 0.0f, 0.0f);
    const long long N = (long long)(rays.size() / 6);

    Out walk(N, F), brute(N, F);
    CHECK(cast(tree, m, rays, 0, walk) == nullptr);
    CHECK(cast(tree, m, rays, 1, brute) == nullptr);
    CHECK(walk.same(brute));
    CHECK(walk.bands_clear(F));
    std::vector<uint8_t> want((size_t)F, 0);
    int hits = 0;
    for (long long n = 0; n < N; ++n) {
        const int f = walk.face[(size_t)n];
        CHECK(f >= -1 && f < F && walk.geom[(size_t)n] == (f >= 0 ? 0 : -1));
        if (f >= 0) {
            ++hits; want[(size_t)f] = 1;
            CHECK(walk.t[(size_t)n] >= 0.0f && walk.t[(size_t)n] < INFINITY);
            const float* nn = &walk.normal[3 * (size_t)n];
            CHECK(fabs((double)nn[0] * nn[0] + (double)nn[1] * nn[1] + (double)nn[2] * nn[2] - 1.0) < 1e-6);
            CHECK(walk.uv[2 * (size_t)n] >= 0.0f && walk.uv[2 * (size_t)n + 1] >= 0.0f && walk.uv[2 * (size_t)n] + walk.uv[2 * (size_t)n + 1] <= 1.0f + 1e-6f);
        } else {
            CHECK(walk.t[(size_t)n] == INFINITY && walk.uv[2 * (size_t)n] == 0.0f && walk.uv[2 * (size_t)n + 1] == 0.0f);
            CHECK(walk.normal[3 * (size_t)n] == 0.0f && walk.normal[3 * (size_t)n + 1] == 0.0f && walk.normal[3 * (size_t)n + 2] == 0.0f);
        }
    }
    for (long long n = valid; n < N; ++n) CHECK(walk.face[(size_t)n] == -1);
    CHECK(memcmp(want.data(), walk.hit.data() + 64, (size_t)F) == 0);

    // occlusion: with tnear <= 0 it is "the nearest hit is at most tfar"; both modes agree for every interval
    const float bounds[4][2] = {{0.0f, INFINITY}, {-1.0f, 0.75f}, {0.5f, 1.5f}, {1.0f, 1.0f}};
    for (auto& b : bounds) {
        std::vector<uint8_t> occ[2];
        for (int mode = 0; mode < 2; ++mode) {
            occ[mode].assign((size_t)N, 7);
            CHECK(mr::occluded_host(tree.data(), tree.size(), V, F, m.v.data(), m.f.data(), 0, N, rays.data(), b[0], b[1], mode, occ[mode].data()) == nullptr);
        }
        CHECK(occ[0] == occ[1]);
        for (long long n = 0; n < N; ++n) {
            const bool in = walk.face[(size_t)n] >= 0 && (double)b[0] <= (double)walk.t[(size_t)n] && (double)walk.t[(size_t)n] <= (double)b[1];
            if (b[0] <= 0.0f) CHECK((occ[0][(size_t)n] != 0) == in);
            CHECK(occ[0][(size_t)n] <= 1 && (!in || occ[0][(size_t)n] == 1));
        }
    }

    // a corrupt header: miss rows, and the call returns.  Corrupt words behind a good header: every call returns, nothing is written out of bounds
    std::vector<char> bad = tree;
    ((Header*)bad.data())->magic = 0;
    Out miss(N, F);
    CHECK(cast(bad, m, rays, 0, miss) == nullptr);
    for (long long n = 0; n < N; ++n) CHECK(miss.face[(size_t)n] == -1 && miss.t[(size_t)n] == INFINITY);
    for (int trial = 0; trial < 4; ++trial) {
        bad = tree;
        int32_t* words = (int32_t*)(bad.data() + HEADER_BYTES);
        const size_t n_words = (bad.size() - HEADER_BYTES) / 4;
        for (int k = 0; k < 2000; ++k) words[lcg(s) % n_words] = (trial & 1) ? (int32_t)lcg(s) : (int32_t)(lcg(s) % (uint32_t)(4 * F + 8)) - 4;
        Out junk(N, F);
        CHECK(cast(bad, m, rays, 0, junk) == nullptr);
        CHECK(junk.bands_clear(F));
        for (long long n = 0; n < N; ++n) CHECK(junk.face[(size_t)n] >= -1 && junk.face[(size_t)n] < F);
        std::vector<uint8_t> occ((size_t)N, 7);
        CHECK(mr::occluded_host(bad.data(), bad.size(), V, F, m.v.data(), m.f.data(), 0, N, rays.data(), 0.0f, INFINITY, 0, occ.data()) == nullptr);
    }
    printf("%s: V %d F %d nodes %u depth %u, %lld rays, %d hits, mode 0 == mode 1\n", name, V, F, h->n_nodes, h->depth, N, hits);
}

int main()
{
    Mesh c = cube();
    check("cube", c, 2000);
    {   // exact ties: the -z side's diagonal, an edge, a corner -> the exact t and the lowest of the tied faces, in both modes
        std::vector<char> tree(tree_bytes(12));
        CHECK(build_tree(8, 12, c.v.data(), c.f.data(), 0, tree.data(), tree.size()) == nullptr);
        std::vector<float> rays;
        push_ray(rays, 0.5f, 0.5f, -2.0f, 0.0f, 0.0f, 1.0f);
        push_ray(rays, -1.0f, -1.0f, 0.5f, 1.0f, 1.0f, 0.0f);
        push_ray(rays, -1.0f, -1.0f, -1.0f, 1.0f, 1.0f, 1.0f);
        push_ray(rays, 0.25f, 0.5f, 0.0f, 0.0f, 0.0f, 1.0f);                          // an origin on a face: t = 0
        push_ray(rays, -1.0f, 0.5f, 0.0f, 1.0f, 0.0f, 0.0f);                          // inside the plane of faces 0 and 1: det == 0, the side x = 0 at t = 1
        for (int mode = 0; mode < 2; ++mode) {
            Out o(5, 12);
            CHECK(cast(tree, c, rays, mode, o) == nullptr);
            CHECK(o.t[0] == 2.0f && o.face[0] == 0 && o.t[1] == 1.0f && o.face[1] == 3 && o.t[2] == 1.0f && o.face[2] == 0);
            CHECK(o.t[3] == 0.0f && o.face[3] >= 0 && o.face[3] <= 1 && o.t[4] == 1.0f && o.face[4] >= 6 && o.face[4] <= 7);
        }
        CHECK(mr::cast_host(tree.data(), tree.size() - 1, 8, 12, c.v.data(), c.f.data(), 0, 5, rays.data(), 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != nullptr);
        CHECK(mr::cast_host(tree.data(), tree.size(), 8, 12, c.v.data(), c.f.data(), 0, 5, rays.data(), 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != nullptr);
        uint8_t occ[5];
        CHECK(mr::occluded_host(tree.data(), tree.size(), 8, 12, c.v.data(), c.f.data(), 0, 5, rays.data(), 1.0f, 0.5f, 0, occ) != nullptr);
        CHECK(mr::occluded_host(tree.data(), tree.size(), 8, 12, c.v.data(), c.f.data(), 0, 5, rays.data(), NAN, 0.5f, 0, occ) != nullptr);
    }
    Mesh flat = c; const int32_t z[9] = {0, 0, 7, 3, 3, 3, 0, 1, 1}; flat.f.insert(flat.f.end(), z, z + 9);          // zero-area faces that name a vertex twice
    check("cube and zero-area faces", flat, 500);
    Mesh one = icosphere(0); one.f.resize(3);
    check("one triangle", one, 500);
    check("icosphere 20", icosphere(0), 1000);
    check("icosphere 1280", icosphere(3), 2000);
    check("icosphere 20480", icosphere(5), 300);
    printf(failures ? "%d checks FAILED\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
