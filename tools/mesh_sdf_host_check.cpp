// Stand-alone host check of the mesh signed distance (youreditableavatar_amd/csrc/tgs_mesh_sdf.hpp): builds the tree of a few meshes, checks its
// invariants, and checks that the tree walk (mode 0) gives the bits of the walk over every face (mode 1).  Host code only, with its own main: it is
// not loaded into Python and needs no device.  Meant to be built with the host sanitizers:
//
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/mesh_sdf_host_check.cpp -o mesh_sdf_host_check
//     ./mesh_sdf_host_check            (prints one line per mesh; exit status 0 when everything holds)
#include "../youreditableavatar_amd/csrc/tgs_mesh_sdf.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

using namespace tgs::msdf;

struct Mesh { std::vector<float> v; std::vector<int32_t> f; };

static Mesh cube()
{
    Mesh m;
    for (int i = 0; i < 8; ++i) { m.v.push_back((i & 1) ? 0.5f : -0.5f); m.v.push_back((i & 2) ? 0.5f : -0.5f); m.v.push_back((i & 4) ? 0.5f : -0.5f); }
    const int q[6][4] = {{0, 2, 3, 1}, {4, 5, 7, 6}, {0, 1, 5, 4}, {2, 6, 7, 3}, {0, 4, 6, 2}, {1, 3, 7, 5}};
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

static void check(const char* name, const Mesh& m, int n_points)
{
    const int V = (int)(m.v.size() / 3), F = (int)(m.f.size() / 3);
    const size_t bytes = tree_bytes((size_t)F);
    std::vector<char> tree(bytes, (char)0x5a), again(bytes, (char)0xa5);
    CHECK(build_tree(V, F, m.v.data(), m.f.data(), 0, tree.data(), bytes) == nullptr);
    CHECK(build_tree(V, F, m.v.data(), m.f.data(), 0, again.data(), bytes) == nullptr);
    CHECK(memcmp(tree.data(), again.data(), bytes) == 0);
    const Header* h = (const Header*)tree.data();
    const Node* nodes = tree_nodes(tree.data());
    const Record* rec = tree_records(tree.data(), (size_t)F);
    CHECK(h->magic == MAGIC && (int)h->n_faces == F && (int)h->n_nodes <= 2 * F && (int)h->depth <= MAX_DEPTH);
    std::vector<int> seen((size_t)F, 0);
    int next_record = 0;
    for (int i = 0; i < (int)h->n_nodes; ++i) {
        CHECK(nodes[i].skip > i && nodes[i].skip <= (int)h->n_nodes);
        if (nodes[i].leaf < 0) continue;
        const int first = nodes[i].leaf >> 3, count = nodes[i].leaf & 7;
        CHECK(first == next_record && count >= 1 && count <= LEAF_FACES && nodes[i].skip == i + 1);
        next_record = first + count;
        for (int r = first; r < first + count; ++r) {
            ++seen[(size_t)rec[r].face];
            for (int k = 0; k < 9; ++k) CHECK(rec[r].v[k] > nodes[i].lo[k % 3] && rec[r].v[k] < nodes[i].hi[k % 3]);
        }
    }
    CHECK(next_record == F);
    for (int f = 0; f < F; ++f) CHECK(seen[(size_t)f] == 1);

    std::vector<float> pts;
    uint32_t s = 12345u;
    for (int k = 0; k < 3 * n_points; ++k) pts.push_back((float)(lcg(s) >> 8) * (2.4f / 16777216.0f) - 1.2f);
    for (int k = 0; k < 9 && k < (int)m.v.size(); ++k) pts.push_back(m.v[(size_t)k]);               // points exactly on vertices
    pts.push_back(NAN); pts.push_back(0.0f); pts.push_back(0.0f);
    pts.push_back(0.0f); pts.push_back(INFINITY); pts.push_back(0.0f);
    const long long N = (long long)(pts.size() / 3);
    std::vector<float> sdf[2], clo[2];
    std::vector<int32_t> face[2];
    std::vector<uint8_t> in[2];
    for (int mode = 0; mode < 2; ++mode) {
        sdf[mode].assign((size_t)N, 7.0f); clo[mode].assign(3 * (size_t)N, 7.0f); face[mode].assign((size_t)N, 7); in[mode].assign((size_t)N, 7);
        CHECK(query_host(tree.data(), bytes, V, F, m.v.data(), m.f.data(), 0, N, pts.data(), mode, sdf[mode].data(), face[mode].data(), clo[mode].data(), in[mode].data()) == nullptr);
    }
    CHECK(memcmp(sdf[0].data(), sdf[1].data(), sizeof(float) * (size_t)N) == 0);
    CHECK(memcmp(clo[0].data(), clo[1].data(), sizeof(float) * 3 * (size_t)N) == 0);
    CHECK(face[0] == face[1] && in[0] == in[1]);
    int inside = 0;
    for (long long n = 0; n < N - 2; ++n) { CHECK(face[0][(size_t)n] >= 0 && sdf[0][(size_t)n] == sdf[0][(size_t)n]); inside += in[0][(size_t)n]; }
    for (long long n = N - 2; n < N; ++n) CHECK(face[0][(size_t)n] == -1 && sdf[0][(size_t)n] != sdf[0][(size_t)n] && in[0][(size_t)n] == 0);
    printf("%s: V %d F %d nodes %u depth %u, %lld points, %d inside, mode 0 == mode 1\n", name, V, F, h->n_nodes, h->depth, N, inside);
}

int main()
{
    Mesh c = cube();
    check("cube", c, 2000);
    CHECK(build_tree(8, 12, c.v.data(), c.f.data(), 0, nullptr, 0) != nullptr);
    std::vector<char> small(tree_bytes(12) - 1);
    CHECK(build_tree(8, 12, c.v.data(), c.f.data(), 0, small.data(), small.size()) != nullptr);
    Mesh bad = c; bad.f[5] = 8;
    std::vector<char> room(tree_bytes(12));
    CHECK(build_tree(8, 12, bad.v.data(), bad.f.data(), 0, room.data(), room.size()) != nullptr);
    bad = c; bad.v[7] = NAN;
    CHECK(build_tree(8, 12, bad.v.data(), bad.f.data(), 0, room.data(), room.size()) != nullptr);
    Mesh flat = c; const int32_t z[3] = {0, 0, 7}; flat.f.insert(flat.f.end(), z, z + 3);           // a zero-area face that names a vertex twice
    check("cube and a zero-area face", flat, 500);
    check("icosphere 20", icosphere(0), 1000);
    check("icosphere 1280", icosphere(3), 2000);
    check("icosphere 20480", icosphere(5), 300);
    printf(failures ? "%d checks FAILED\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
