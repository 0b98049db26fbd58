// marching_cubes.hpp -- the reference's marchingCubes(Model*, scale, translation, threshold,
// outFileName) (src/MarchingCubes.h:596, src/MarchingCubes.cpp:8-31) over the GPU library:
// same name, arguments, defaults, return value, log lines and -- byte for byte -- the same
// OFF file (pinned against the reference's own Data/box_dataset/generated_models/1.off,
// tests/test_mc_off.py).
//
// The reference visits all (X+1)(Y+1)(Z+1) cells and reads eight voxels per cell through
// Model::get, although only cells cut by the surface emit anything (Polygonise returns at once
// when edgeTable[cubeIdx] == 0, src/MarchingCubes.h:486-488).  Here the GPU finds exactly those
// cells (arvx_mc_cells: cube index and position, in the order the reference's loops reach
// them -- x outermost, z innermost, each from -1) and the host triangulates that list with the
// reference's rules:
//   * a cut edge's vertex snaps to the corner that belongs to the model when the other one has
//     w == 0, and takes that corner's colour (VertexInterp, :428-441); otherwise position and
//     colour are interpolated, except that MODEL_COLOR / UNSEEN_COLOR are never blended in
//     (:443-467);
//   * every triangle gets three fresh vertices (ProcessVoxel, :561-568), and its third corner's
//     COLOUR is the second corner's (`i + 1` instead of `i + 2`, :506 -- kept);
//   * face colour = round((c0 + c1 + c2) / 3) per channel in fp32 (MeanColorFloats, :414-416);
//   * OFF text as SimpleMesh::WriteMesh prints it (:60-87): default ostream float format,
//     vertex * scaleFactor + translation evaluated in fp32.
#ifndef ARVX_MARCHING_CUBES_HPP
#define ARVX_MARCHING_CUBES_HPP

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <map>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "arvx/host_pool.hpp"
#include "arvx/mc_tables.hpp"
#include "arvx/mesh_texture.hpp"
#include "arvx/voxel_carving.hpp"

namespace arvx {

struct Triangle {  // src/MarchingCubes.h:19-31
    unsigned int idx0, idx1, idx2;
    unsigned int r, g, b;
};

// (the two arrays live in recycled page-locked memory, include/arvx/host_pool.hpp: a mesh of
// 1.3 M triangles is 77 MB that the device writes in the arrays' own layout)
class SimpleMesh {  // src/MarchingCubes.h:33-92
   public:
    unsigned int AddVertex(const Vec3f &vertex) {
        m_vertices.push_back(vertex);
        return (unsigned int)m_vertices.size() - 1;
    }
    unsigned int AddFace(unsigned int idx0, unsigned int idx1, unsigned int idx2, unsigned int r = 0,
                         unsigned int g = 0, unsigned int b = 0) {
        m_triangles.push_back(Triangle{idx0, idx1, idx2, r, g, b});
        return (unsigned int)m_triangles.size() - 1;
    }
    HostVector<Vec3f> &GetVertices() { return m_vertices; }
    HostVector<Triangle> &GetTriangles() { return m_triangles; }
    const HostVector<Vec3f> &GetVertices() const { return m_vertices; }
    const HostVector<Triangle> &GetTriangles() const { return m_triangles; }

    // The reference ends every line with std::endl (one flush per line); '\n' and one flush at
    // the end give the same bytes.
    bool WriteMesh(const std::string &filename, float scaleFactor = 1.f,
                   Vec3f translation = Vec3f(0, 0, 0)) {
        std::ofstream outFile(filename);
        if (!outFile.is_open()) return false;
        outFile << "OFF" << '\n';
        outFile << m_vertices.size() << " " << m_triangles.size() << " 0" << '\n';
        for (const Vec3f &p : m_vertices) {
            // fp32 multiply, then fp32 add (two statements: no contraction into an fma)
            volatile float px = p.x() * scaleFactor, py = p.y() * scaleFactor,
                           pz = p.z() * scaleFactor;
            const float ox = px + translation.x(), oy = py + translation.y(),
                        oz = pz + translation.z();
            outFile << ox << " " << oy << " " << oz << '\n';
        }
        for (const Triangle &t : m_triangles)
            outFile << "3 " << t.idx0 << " " << t.idx1 << " " << t.idx2 << " " << t.r << " " << t.g
                    << " " << t.b << '\n';
        outFile.flush();
        const bool ok = outFile.good();
        outFile.close();
        return ok;
    }

   private:
    HostVector<Vec3f> m_vertices;
    HostVector<Triangle> m_triangles;
};

struct McCell {
    int x, y, z;    // base corner of the cell, each in [-1, size)
    int cubeIndex;  // Polygonise's cubeIdx (src/MarchingCubes.h:479-484), never 0 or 255
};

// The cells marchingCubes() triangulates, in its visiting order, found on the GPU.
// A corner counts as outside when its w < threshold (:481); the reference's own pipeline only
// ever holds w in {0, 1} and passes 0.5.
inline std::vector<McCell> marchingCubesCells(Model &model, float threshold = 0.5f) {
    static_assert(sizeof(McCell) == 4 * sizeof(int32_t), "McCell is the C-ABI's 4-int record");
    // w >= 0 everywhere the grid is, and 0 outside it: with threshold <= 0 no corner is outside
    if (!(threshold > 0.f)) return {};
    bool on_device = false;
    const std::vector<uint8_t> inside = model.inside_state(threshold, on_device);
    arvx_ctx *ctx = nullptr;
    struct Guard {
        arvx_ctx *c;
        ~Guard() {
            if (c) arvx_ctx_destroy(c);
        }
    } guard{nullptr};
    if (on_device) {  // "inside" is the occupancy the model's context already holds
        ctx = model.device_for_reading();
    } else {  // fractional w: a thresholded plane of its own, in a context of its own
        detail::check(arvx_ctx_create(&ctx, 0, model.getX(), model.getY(), model.getZ(),
                                      model.getSize()),
                      "arvx_ctx_create");
        guard.c = ctx;
        detail::check(arvx_state_upload(ctx, inside.data()), "arvx_state_upload");
    }
    int64_t n = 0;
    detail::check(arvx_mc_cells(ctx, &n), "arvx_mc_cells");
    std::vector<McCell> cells((size_t)n);
    if (n) detail::check(arvx_mc_cells_download(ctx, (int32_t *)cells.data()),
                         "arvx_mc_cells_download");
    return cells;
}

namespace mc {

struct Interp {
    Vec3f coord, color;
};

inline bool is_default_color(const Vec3f &c) {  // MODEL_COLOR / UNSEEN_COLOR, src/Model.h:90-91
    return c == Vec3f(50, 168, 141) || c == Vec3f(204, 0, 0);
}

// src/MarchingCubes.h:428-468
inline Interp vertex_interp(float threshold, const Vec3f &point0, const Vec4f &val0,
                            const Vec3f &point1, const Vec4f &val1) {
    Interp ret;
    if (val0.w() == 0.0f && val1.w() != 0.0f) {  // corner 0 is not part of the model
        ret.color = Vec3f(val1.x(), val1.y(), val1.z());
        ret.coord = point1;
        return ret;
    }
    if (val0.w() != 0.0f && val1.w() == 0.0f) {
        ret.color = Vec3f(val0.x(), val0.y(), val0.z());
        ret.coord = point0;
        return ret;
    }
    const float f = (val0.w() == val1.w()) ? 0.5f : (threshold - val0.w()) / (val1.w() - val0.w());
    const float g = 1 - f;
    const Vec3f col0(val0.x(), val0.y(), val0.z()), col1(val1.x(), val1.y(), val1.z());
    for (int k = 0; k < 3; ++k) {
        volatile float a = g * point0[k], b = f * point1[k];  // (1-f)*p0 + f*p1, unfused
        ret.coord[k] = a + b;
    }
    if (is_default_color(col0)) {
        ret.color = col1;
    } else if (is_default_color(col1)) {
        ret.color = col0;
    } else {
        for (int k = 0; k < 3; ++k) {
            volatile float a = g * col0[k], b = f * col1[k];
            ret.color[k] = a + b;
        }
    }
    return ret;
}

// MeanColorFloats, src/MarchingCubes.h:414-416
inline unsigned int mean_color(float c1, float c2, float c3) {
    volatile float s = c1 + c2;
    s = s + c3;
    return (unsigned int)std::round(s / 3);
}

}  // namespace mc

// One cell: Polygonise + ProcessVoxel of the reference (src/MarchingCubes.h:478-511, 532-578).
// Returns whether the cell emitted a triangle.
inline bool ProcessVoxel(Model *model, int x, int y, int z, SimpleMesh *mesh, float threshold) {
    static const int corner[8][3] = {{1, 0, 0}, {0, 0, 0}, {0, 1, 0}, {1, 1, 0},
                                     {1, 0, 1}, {0, 0, 1}, {0, 1, 1}, {1, 1, 1}};  // :537-552
    Vec4f val[8];
    Vec3f p[8];
    int cubeIdx = 0;
    for (int i = 0; i < 8; ++i) {
        const int cx = x + corner[i][0], cy = y + corner[i][1], cz = z + corner[i][2];
        val[i] = model->get(cx, cy, cz);
        p[i] = Vec3f((float)cx, (float)cy, (float)cz);
        if (val[i].w() < threshold) cubeIdx |= 1 << i;
    }
    const int edges = mc::edge_mask(cubeIdx);
    if (edges == 0) return false;
    mc::Interp vert[12];
    for (int e = 0; e < 12; ++e)
        if (edges & (1 << e))
            vert[e] = mc::vertex_interp(threshold, p[e % 8], val[e % 8], p[mc::kSecondCorner[e]],
                                        val[mc::kSecondCorner[e]]);
    const char *tri = mc::kTriangles[cubeIdx];
    bool any = false;
    for (; tri[0]; tri += 3) {
        const mc::Interp &a = vert[mc::hex_digit(tri[0])], &b = vert[mc::hex_digit(tri[1])],
                         &c = vert[mc::hex_digit(tri[2])];
        const unsigned int h0 = mesh->AddVertex(a.coord);
        const unsigned int h1 = mesh->AddVertex(b.coord);
        const unsigned int h2 = mesh->AddVertex(c.coord);
        // the third corner's colour is the second's: src/MarchingCubes.h:506 reads [i + 1]
        const Vec3f &c0 = a.color, &c1 = b.color, &c2 = b.color;
        mesh->AddFace(h0, h1, h2, mc::mean_color(c0.x(), c1.x(), c2.x()),
                      mc::mean_color(c0.y(), c1.y(), c2.y()), mc::mean_color(c0.z(), c1.z(), c2.z()));
        any = true;
    }
    return any;
}

namespace detail {
// The model's context, ready for the device mesh of a model whose w are all 0 or 1: painted voxels
// are derived on the device when the paint is exactly "not seen" (*apply_unseen = 1), else carried
// by the byte plane (bit2); the colours are on the device.
inline arvx_ctx *mesh_context(Model *model, int &apply_unseen) {
    arvx_ctx *ctx = model->device_for_reading();
    const bool painted = model->painted();
    if (painted && !model->paint_is_unseen()) {
        const std::vector<uint8_t> st = model->byte_state();
        detail::check(arvx_state_upload(ctx, st.data()), "arvx_state_upload");
        model->set_colors_on_device(false);
    }
    if (!model->colors_on_device()) {
        std::vector<int64_t> idx;
        std::vector<float> rgb;
        (void)model->sorted_colors(idx, rgb);  // (w is 0 or 1 here)
        detail::check(arvx_colors_upload(ctx, (int64_t)idx.size(), idx.data(), rgb.data()),
                      "arvx_colors_upload");
        model->set_colors_on_device(true);
    }
    apply_unseen = (painted && model->paint_is_unseen()) ? 1 : 0;
    return ctx;
}
}  // namespace detail

// The mesh marchingCubes() writes, without writing it.  When every w of the model is 0 or 1
// (all the reference's own pipeline produces) the triangles come from the device
// (arvx_mc_mesh: state, colour list and closure result are already there); a model with
// fractional w is triangulated on the host from the device's cell list.
inline SimpleMesh marchingCubesMesh(Model *model, float threshold = 0.5f) {
    SimpleMesh mesh;
    if (!(threshold > 0.f)) return mesh;
#ifdef ARVX_HOST_TRACE  // diagnostic builds: where the host time of this call goes
    using TraceClock = std::chrono::steady_clock;
    auto trace_t = TraceClock::now();
    auto trace = [&](const char *what) {
        const auto now = TraceClock::now();
        std::fprintf(stderr, "    [mesh] %-18s %.3f ms\n", what,
                     std::chrono::duration<double, std::milli>(now - trace_t).count());
        trace_t = now;
    };
#define ARVX_TRACE(what) trace(what)
#else
#define ARVX_TRACE(what) (void)0
#endif
    bool on_device = false;
    (void)model->inside_state(threshold, on_device);
    ARVX_TRACE("inside_state");
    if (!on_device) {
        for (const McCell &c : marchingCubesCells(*model, threshold))
            ProcessVoxel(model, c.x, c.y, c.z, &mesh, threshold);
        return mesh;
    }
    int apply_unseen = 0;
    arvx_ctx *ctx = detail::mesh_context(model, apply_unseen);
    ARVX_TRACE("context + colours");
    int64_t n = 0;
    detail::check(arvx_mc_mesh(ctx, apply_unseen, &n), "arvx_mc_mesh");
    ARVX_TRACE("arvx_mc_mesh");
    // the device writes both arrays in the mesh's own layout: a triangle's three corners as
    // nine floats, its face as (3t, 3t+1, 3t+2, r, g, b)
    static_assert(sizeof(Vec3f) == 3 * sizeof(float), "Vec3f is three packed floats");
    static_assert(sizeof(Triangle) == 6 * sizeof(uint32_t), "Triangle is six packed uints");
    HostVector<Vec3f> &mv = mesh.GetVertices();
    HostVector<Triangle> &mt = mesh.GetTriangles();
    mv.resize((size_t)n * 3);  // (recycled memory, not zeroed: host_pool.hpp)
    mt.resize((size_t)n);
    ARVX_TRACE("resize");
    if (n) detail::check(arvx_mc_mesh_download_faces(ctx, mv[0].data(), &mt[0].idx0),
                         "arvx_mc_mesh_download_faces");
    ARVX_TRACE("download");
#undef ARVX_TRACE
    return mesh;
}

namespace detail {
// marchingCubes' frame around a mesh builder: log lines, Benchmark stage, WriteMesh
template <class Build>
inline bool marching_cubes_write(Model *model, float scale, Vec3f translation, float threshold,
                                 const std::string &outFileName, Build build) {
    std::cout << "LOG - MC: starting to process Voxels." << std::endl;
    detail::timing(kStageMarchingCubes, true);
    SimpleMesh mesh = build(model, threshold);
    detail::timing(kStageMarchingCubes, false);
    std::cout << "LOG - MC: voxel processing completed.\n Writing mesh..." << std::endl;
    volatile float factor = scale * model->getSize();
    if (!mesh.WriteMesh(outFileName, factor, translation)) {
        std::cout << "ERR - MC: unable to write output file!" << std::endl;
        return false;
    }
    std::cout << "LOG - MC: Mesh written, marchingCubes completed." << std::endl;
    return true;
}
}  // namespace detail

inline bool marchingCubes(Model *model, float scale = 1.0f, Vec3f translation = Vec3f(0, 0, 0),
                          float threshold = 0.5f, std::string outFileName = "out/mesh.off") {
    return detail::marching_cubes_write(model, scale, translation, threshold, outFileName,
                                        [](Model *m, float t) { return marchingCubesMesh(m, t); });
}

// ---- welded mesh (an extension beyond the reference) -------------------------------------------
//
// The definition of arvx_mc_mesh_welded (include/arvx/arvx.h) applied to any mesh: the distinct
// vertex positions, compared as float values, ascending by (z, y, x); the same triangles in the
// same order with their indices into that list and their colours; degenerate triangles kept.
inline SimpleMesh weldMesh(const SimpleMesh &mesh) {
    const HostVector<Vec3f> &v = mesh.GetVertices();
    const HostVector<Triangle> &tris = mesh.GetTriangles();
    auto before = [&v](unsigned int a, unsigned int b) {
        const Vec3f &p = v[a], &q = v[b];
        if (p.z() != q.z()) return p.z() < q.z();
        if (p.y() != q.y()) return p.y() < q.y();
        return p.x() < q.x();
    };
    std::vector<unsigned int> order(v.size()), index(v.size());
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), before);
    SimpleMesh out;
    unsigned int next = 0;
    for (size_t k = 0; k < order.size(); ++k) {
        if (k == 0 || before(order[k - 1], order[k])) next = out.AddVertex(v[order[k]]);
        index[order[k]] = next;
    }
    out.GetTriangles().reserve(tris.size());
    for (const Triangle &t : tris)
        out.AddFace(index[t.idx0], index[t.idx1], index[t.idx2], t.r, t.g, t.b);
    return out;
}

// marchingCubesMesh with shared vertices: weldMesh(marchingCubesMesh(model, threshold)).  When
// every w is 0 or 1 the device builds it directly (arvx_mc_mesh_welded: 12 bytes per vertex and
// 24 per triangle cross PCIe instead of 60 per triangle); a model with fractional w -- vertices
// interpolated, not snapped -- is welded on the host.
inline SimpleMesh marchingCubesMeshWelded(Model *model, float threshold = 0.5f) {
    if (!(threshold > 0.f)) return SimpleMesh();
    bool on_device = false;
    (void)model->inside_state(threshold, on_device);
    if (!on_device) return weldMesh(marchingCubesMesh(model, threshold));
    int apply_unseen = 0;
    arvx_ctx *ctx = detail::mesh_context(model, apply_unseen);
    int64_t nv = 0, nt = 0;
    detail::check(arvx_mc_mesh_welded(ctx, apply_unseen, &nv, &nt), "arvx_mc_mesh_welded");
    SimpleMesh mesh;
    HostVector<Vec3f> &mv = mesh.GetVertices();
    HostVector<Triangle> &mt = mesh.GetTriangles();
    mv.resize((size_t)nv);  // (recycled memory, not zeroed: host_pool.hpp)
    mt.resize((size_t)nt);
    detail::check(arvx_mc_mesh_welded_download(ctx, nv ? mv[0].data() : nullptr,
                                                 nt ? &mt[0].idx0 : nullptr, nullptr),
                  "arvx_mc_mesh_welded_download");
    return mesh;
}

// marchingCubes writing the welded mesh: same arguments, log lines and Benchmark stage.
inline bool marchingCubesWelded(Model *model, float scale = 1.0f, Vec3f translation = Vec3f(0, 0, 0),
                                float threshold = 0.5f, std::string outFileName = "out/mesh.off") {
    return detail::marching_cubes_write(model, scale, translation, threshold, outFileName,
                                        [](Model *m, float t) { return marchingCubesMeshWelded(m, t); });
}

// ---- render (an extension beyond the reference) -------------------------------------------------
//
// The welded mesh's vertex voxels drawn into a camera view on the device (arvx_render, defined in
// include/arvx/arvx.h): M is the camera, row-major 3 x 4, world -> pixel; background, if given, is
// a tightly packed H x W BGR image that shows where no voxel covers a pixel.  id holds indices into
// the welded mesh's vertex list (-1: none), depth the winner's a2 (+inf: none).
struct RenderedView {
    std::vector<uint8_t> bgr;
    std::vector<float> depth;
    std::vector<int32_t> id;
    int W = 0, H = 0;
};

// Renders the welded mesh the model's context holds; builds it first (as marchingCubesMeshWelded
// does) ONLY if the context has none.  The context's welded mesh lives until the next welded mesh
// is built, not until the model changes: after marchingCubesMeshWelded, a carve, handleUnseen, a
// closure or a new colouring leaves it in place, and this call then draws that older mesh (ids and
// colours are those of that mesh, which is what its downloaded arrays hold).  To draw the model as
// it now is, call marchingCubesMeshWelded again first.  A model with fractional w has no welded
// mesh on the device: the call throws.
inline RenderedView renderWelded(Model *model, const float M[12], int W, int H,
                                 const uint8_t *background = nullptr) {
    arvx_ctx *ctx = model->device_for_reading();
    const size_t stride = (size_t)(W > 0 ? W : 0) * 3;
    int rc = arvx_render(ctx, M, W, H, background, stride);
    if (rc == ARVX_ERR_STATE) {  // no welded mesh yet
        bool on_device = false;
        (void)model->inside_state(0.5f, on_device);
        if (on_device) {
            int apply_unseen = 0;
            ctx = detail::mesh_context(model, apply_unseen);
            int64_t nv = 0, nt = 0;
            detail::check(arvx_mc_mesh_welded(ctx, apply_unseen, &nv, &nt), "arvx_mc_mesh_welded");
            rc = arvx_render(ctx, M, W, H, background, stride);
        }
    }
    detail::check(rc, "arvx_render");
    RenderedView out;
    out.W = W;
    out.H = H;
    out.bgr.resize((size_t)W * H * 3);
    out.depth.resize((size_t)W * H);
    out.id.resize((size_t)W * H);
    detail::check(arvx_render_download(ctx, out.bgr.data(), out.depth.data(), out.id.data()),
                  "arvx_render_download");
    return out;
}

// ---- smoothed mesh (an extension beyond the reference) ------------------------------------------
//
// The definition of arvx_mc_mesh_smooth (include/arvx/arvx.h) applied to any welded mesh on the
// host: Taubin smoothing with (iterations, lambda, mu), then -- if normals is not null -- the unit
// vertex normals of the result.  Returns the mesh with the smoothed positions and the same
// triangles.  (Compiled with -ffp-contract=off, as the tools and tests are, this is bit for bit
// what the device computes.)
inline SimpleMesh smoothMesh(const SimpleMesh &welded, int iterations, float lambda = 0.5f,
                             float mu = -0.53f, HostVector<Vec3f> *normals = nullptr) {
    const HostVector<Triangle> &tris = welded.GetTriangles();
    const size_t V = welded.GetVertices().size();
    // N(i): the other corners of i's faces, each once, ascending
    std::vector<std::vector<unsigned int>> nbr(V);
    for (const Triangle &t : tris) {
        const unsigned int c[3] = {t.idx0, t.idx1, t.idx2};
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b)
                if (c[a] != c[b]) nbr[c[a]].push_back(c[b]);
    }
    for (std::vector<unsigned int> &n : nbr) {
        std::sort(n.begin(), n.end());
        n.erase(std::unique(n.begin(), n.end()), n.end());
    }
    std::vector<Vec3f> p(welded.GetVertices().begin(), welded.GetVertices().end()), next(V);
    for (int s = 0; s < 2 * iterations; ++s) {
        const float f = (s & 1) ? mu : lambda;
        for (size_t i = 0; i < V; ++i) {
            if (nbr[i].empty()) {
                next[i] = p[i];
                continue;
            }
            const float k = (float)nbr[i].size();
            for (int c = 0; c < 3; ++c) {
                float sum = 0.f;
                for (unsigned int j : nbr[i]) sum = sum + p[j][c];
                const float d = sum / k - p[i][c];
                const float fd = f * d;
                next[i][c] = p[i][c] + fd;
            }
        }
        p.swap(next);
    }
    SimpleMesh out;
    HostVector<Vec3f> &ov = out.GetVertices();
    ov.resize(V);
    std::copy(p.begin(), p.end(), ov.begin());
    HostVector<Triangle> &ot = out.GetTriangles();
    ot.resize(tris.size());
    std::copy(tris.begin(), tris.end(), ot.begin());
    if (normals) {
        std::vector<Vec3f> n(V);
        for (const Triangle &t : tris) {  // ascending t; each face once per corner vertex
            const Vec3f &q0 = p[t.idx0], &q1 = p[t.idx1], &q2 = p[t.idx2];
            const float ax = q2.x() - q0.x(), ay = q2.y() - q0.y(), az = q2.z() - q0.z();
            const float bx = q1.x() - q0.x(), by = q1.y() - q0.y(), bz = q1.z() - q0.z();
            const float l0 = ay * bz, r0 = az * by, l1 = az * bx, r1 = ax * bz, l2 = ax * by, r2 = ay * bx;
            const Vec3f c(l0 - r0, l1 - r1, l2 - r2);
            const unsigned int v[3] = {t.idx0, t.idx1, t.idx2};
            for (int k = 0; k < 3; ++k) {
                if ((k > 0 && v[k] == v[0]) || (k > 1 && v[k] == v[1])) continue;
                for (int e = 0; e < 3; ++e) n[v[k]][e] = n[v[k]][e] + c[e];
            }
        }
        normals->resize(V);
        for (size_t i = 0; i < V; ++i) {
            const float xx = n[i].x() * n[i].x(), yy = n[i].y() * n[i].y(), zz = n[i].z() * n[i].z();
            const float l = std::sqrt((xx + yy) + zz);
            (*normals)[i] = l == 0.f ? Vec3f(0, 0, 0) : Vec3f(n[i].x() / l, n[i].y() / l, n[i].z() / l);
        }
    }
    return out;
}

// marchingCubesMeshWelded, smoothed: smoothMesh(marchingCubesMeshWelded(model, threshold), ...).
// When every w is 0 or 1 the device smooths the welded mesh it has just built
// (arvx_mc_mesh_smooth); a model with fractional w is smoothed on the host.
inline SimpleMesh marchingCubesMeshSmoothed(Model *model, float threshold = 0.5f, int iterations = 1,
                                            float lambda = 0.5f, float mu = -0.53f,
                                            HostVector<Vec3f> *normals = nullptr) {
    if (!(threshold > 0.f)) {
        if (normals) normals->clear();
        return SimpleMesh();
    }
    bool on_device = false;
    (void)model->inside_state(threshold, on_device);
    if (!on_device) return smoothMesh(marchingCubesMeshWelded(model, threshold), iterations, lambda, mu, normals);
    int apply_unseen = 0;
    arvx_ctx *ctx = detail::mesh_context(model, apply_unseen);
    int64_t nv = 0, nt = 0;
    detail::check(arvx_mc_mesh_welded(ctx, apply_unseen, &nv, &nt), "arvx_mc_mesh_welded");
    detail::check(arvx_mc_mesh_smooth(ctx, iterations, lambda, mu), "arvx_mc_mesh_smooth");
    SimpleMesh mesh;
    HostVector<Vec3f> &mv = mesh.GetVertices();
    HostVector<Triangle> &mt = mesh.GetTriangles();
    mv.resize((size_t)nv);  // (recycled memory, not zeroed: host_pool.hpp)
    mt.resize((size_t)nt);
    // (the welded download needs a vertex array: the lattice positions land where the smoothed
    // ones then go)
    detail::check(arvx_mc_mesh_welded_download(ctx, nv ? mv[0].data() : nullptr,
                                                 nt ? &mt[0].idx0 : nullptr, nullptr),
                  "arvx_mc_mesh_welded_download");
    if (normals) normals->resize((size_t)nv);
    detail::check(arvx_mc_mesh_smooth_download(ctx, nv ? mv[0].data() : nullptr,
                                                 (normals && nv) ? (*normals)[0].data() : nullptr),
                  "arvx_mc_mesh_smooth_download");
    return mesh;
}

// marchingCubes writing the smoothed welded mesh: marchingCubes' arguments, log lines and
// Benchmark stage, then the smoothing's.
inline bool marchingCubesSmoothed(Model *model, float scale = 1.0f, Vec3f translation = Vec3f(0, 0, 0),
                                  float threshold = 0.5f, std::string outFileName = "out/mesh.off",
                                  int iterations = 1, float lambda = 0.5f, float mu = -0.53f) {
    return detail::marching_cubes_write(model, scale, translation, threshold, outFileName,
                                        [=](Model *m, float t) {
                                            return marchingCubesMeshSmoothed(m, t, iterations, lambda, mu);
                                        });
}

// ---- decimated mesh (an extension beyond the reference) -----------------------------------------
//
// The definition of arvx_mc_mesh_decimate (include/arvx/arvx.h) on the host, for a welded mesh
// whose vertices lie on the lattice (for any other mesh the cluster of a vertex is floor(p) / cell,
// floored, and the clusters are taken in ascending (z, y, x)): vertices that fall into the same
// cube of cell^3 voxels become one, at the mean of `smoothed`'s positions when it is given (same
// vertex count; the clusters always come from `welded`) or of their own; faces that lose a corner
// go, of the faces with the same corner set the first stays.  members (may be null): welded
// vertices per decimated vertex; map (may be null): the decimated index of every welded vertex.
// (Compiled with -ffp-contract=off, as the tools and tests are, this is bit for bit what the device
// computes.)
inline SimpleMesh decimateMesh(const SimpleMesh &welded, int cell, const SimpleMesh *smoothed = nullptr,
                               std::vector<int32_t> *members = nullptr, std::vector<int32_t> *map = nullptr) {
    if (cell < 1) throw std::invalid_argument("decimateMesh: cell must be >= 1");
    const HostVector<Vec3f> &lattice = welded.GetVertices();
    const HostVector<Vec3f> &q = smoothed ? smoothed->GetVertices() : lattice;
    const size_t V = lattice.size();
    if (q.size() != V) throw std::invalid_argument("decimateMesh: the smoothed mesh has other vertices");
    auto cluster_of = [cell](float p) {
        const long long l = (long long)std::floor(p);
        return l >= 0 ? l / cell : -((-l + cell - 1) / cell);
    };
    // clusters in ascending (z, y, x); their members arrive in ascending vertex index
    std::map<std::array<long long, 3>, std::vector<unsigned int>> clusters;
    for (size_t i = 0; i < V; ++i)
        clusters[{cluster_of(lattice[i].z()), cluster_of(lattice[i].y()), cluster_of(lattice[i].x())}].push_back(
            (unsigned int)i);
    SimpleMesh out;
    std::vector<unsigned int> index(V);
    if (members) members->clear();
    for (const auto &c : clusters) {
        const float n = (float)c.second.size();
        Vec3f s(0, 0, 0);
        for (unsigned int i : c.second)
            for (int k = 0; k < 3; ++k) s[k] = s[k] + q[i][k];
        const unsigned int at = out.AddVertex(Vec3f(s.x() / n, s.y() / n, s.z() / n));
        for (unsigned int i : c.second) index[i] = at;
        if (members) members->push_back((int32_t)c.second.size());
    }
    if (map) map->assign(index.begin(), index.end());
    std::map<std::array<unsigned int, 3>, bool> seen;
    for (const Triangle &t : welded.GetTriangles()) {
        const unsigned int a = index[t.idx0], b = index[t.idx1], c = index[t.idx2];
        if (a == b || b == c || a == c) continue;
        std::array<unsigned int, 3> key{a, b, c};
        std::sort(key.begin(), key.end());
        if (!seen.emplace(key, true).second) continue;
        out.AddFace(a, b, c, t.r, t.g, t.b);
    }
    return out;
}

// marchingCubesMeshWelded, decimated: decimateMesh of the welded mesh (iterations = 0) or of the
// welded mesh with smoothMesh's positions (iterations > 0).  When every w is 0 or 1 the device
// does all of it (arvx_mc_mesh_welded, arvx_mc_mesh_smooth, arvx_mc_mesh_decimate) and only the
// decimated mesh crosses PCIe; a model with fractional w is decimated on the host.
inline SimpleMesh marchingCubesMeshDecimated(Model *model, float threshold = 0.5f, int cell = 2,
                                             int iterations = 0, float lambda = 0.5f, float mu = -0.53f) {
    if (!(threshold > 0.f)) return SimpleMesh();
    bool on_device = false;
    (void)model->inside_state(threshold, on_device);
    if (!on_device) {
        const SimpleMesh welded = marchingCubesMeshWelded(model, threshold);
        if (iterations <= 0) return decimateMesh(welded, cell);
        const SimpleMesh smoothed = smoothMesh(welded, iterations, lambda, mu);
        return decimateMesh(welded, cell, &smoothed);
    }
    int apply_unseen = 0;
    arvx_ctx *ctx = detail::mesh_context(model, apply_unseen);
    int64_t nv = 0, nt = 0, dv = 0, dt = 0;
    detail::check(arvx_mc_mesh_welded(ctx, apply_unseen, &nv, &nt), "arvx_mc_mesh_welded");
    if (iterations > 0) detail::check(arvx_mc_mesh_smooth(ctx, iterations, lambda, mu), "arvx_mc_mesh_smooth");
    detail::check(arvx_mc_mesh_decimate(ctx, cell, iterations > 0 ? ARVX_DECIMATE_SMOOTHED : ARVX_DECIMATE_LATTICE,
                                        &dv, &dt),
                  "arvx_mc_mesh_decimate");
    SimpleMesh mesh;
    HostVector<Vec3f> &mv = mesh.GetVertices();
    HostVector<Triangle> &mt = mesh.GetTriangles();
    mv.resize((size_t)dv);  // (recycled memory, not zeroed: host_pool.hpp)
    mt.resize((size_t)dt);
    detail::check(arvx_mc_mesh_decimate_download(ctx, dv ? mv[0].data() : nullptr, dt ? &mt[0].idx0 : nullptr,
                                                 nullptr, nullptr, nullptr),
                  "arvx_mc_mesh_decimate_download");
    return mesh;
}

// marchingCubes writing the decimated welded mesh: marchingCubes' arguments, log lines and
// Benchmark stage, then the cell and the smoothing's arguments.
inline bool marchingCubesDecimated(Model *model, float scale = 1.0f, Vec3f translation = Vec3f(0, 0, 0),
                                   float threshold = 0.5f, std::string outFileName = "out/mesh.off",
                                   int cell = 2, int iterations = 0, float lambda = 0.5f, float mu = -0.53f) {
    return detail::marching_cubes_write(model, scale, translation, threshold, outFileName,
                                        [=](Model *m, float t) {
                                            return marchingCubesMeshDecimated(m, t, cell, iterations, lambda, mu);
                                        });
}

// ---- refined mesh (an extension beyond the reference) --------------------------------------------
//
// Marching cubes with one vertex per cut edge, placed where the edge leaves the visual hull of the
// views' masks by `bisections` bisection steps (arvx_mc_mesh_refined, defined in include/arvx/arvx.h;
// 0: plain edge midpoints).  The views are bound as carveVotes binds them -- matrices and masks; they
// need not be the views the model was carved with, though only those explain its surface.  The
// triangles, their order and their colours are marchingCubesMesh's; the vertices are shared.  The
// device does all of it and there is no host route: a model with fractional w, whose vertices the
// reference interpolates by w, is refused with an exception.
inline SimpleMesh marchingCubesMeshRefined(const Intrinsics &intr, Model *model, const std::vector<View> &views,
                                           int bisections = 6, float threshold = 0.5f) {
    if (!(threshold > 0.f)) return SimpleMesh();
    bool on_device = false;
    (void)model->inside_state(threshold, on_device);
    if (!on_device)
        throw Error(ARVX_ERR_STATE, "marchingCubesMeshRefined: the model has voxels with fractional w; the refined "
                                    "mesh is built on the device from models whose w are all 0 or 1");
    (void)detail::bind_views(intr, *model, views, false);
    model->set_colors_on_device(false);  // (arvx_set_views drops the context's colour list)
    int apply_unseen = 0;
    arvx_ctx *ctx = detail::mesh_context(model, apply_unseen);
    int64_t nv = 0, nt = 0;
    detail::check(arvx_mc_mesh_refined(ctx, apply_unseen, bisections, &nv, &nt), "arvx_mc_mesh_refined");
    SimpleMesh mesh;
    HostVector<Vec3f> &mv = mesh.GetVertices();
    HostVector<Triangle> &mt = mesh.GetTriangles();
    mv.resize((size_t)nv);  // (recycled memory, not zeroed: host_pool.hpp)
    mt.resize((size_t)nt);
    detail::check(arvx_mc_mesh_refined_download(ctx, nv ? mv[0].data() : nullptr, nt ? &mt[0].idx0 : nullptr,
                                                nullptr, nullptr, nullptr),
                  "arvx_mc_mesh_refined_download");
    return mesh;
}

// marchingCubes writing the refined mesh: the views and the bisections, then marchingCubes'
// arguments, log lines and Benchmark stage.
inline bool marchingCubesRefined(const Intrinsics &intr, Model *model, const std::vector<View> &views,
                                 int bisections = 6, float scale = 1.0f, Vec3f translation = Vec3f(0, 0, 0),
                                 float threshold = 0.5f, std::string outFileName = "out/mesh.off") {
    return detail::marching_cubes_write(model, scale, translation, threshold, outFileName,
                                        [&](Model *m, float t) {
                                            return marchingCubesMeshRefined(intr, m, views, bisections, t);
                                        });
}

// ---- triangle render (an extension beyond the reference) -----------------------------------------
//
// A mesh's triangles drawn into a camera view on the device with a depth buffer (arvx_render_mesh,
// defined in include/arvx/arvx.h): M, W, H and background as for renderWelded; light, if given, is 3
// floats along the voxel axes that shade every face by the angle between its normal and the light
// ({M[9], M[8], -M[10]}: a light at the camera).  id holds indices into the mesh's triangle list.
namespace detail {
inline RenderedView rendered_view(arvx_ctx *ctx, int W, int H) {
    RenderedView out;
    out.W = W;
    out.H = H;
    out.bgr.resize((size_t)W * H * 3);
    out.depth.resize((size_t)W * H);
    out.id.resize((size_t)W * H);
    check(arvx_render_download(ctx, out.bgr.data(), out.depth.data(), out.id.data()), "arvx_render_download");
    return out;
}
}  // namespace detail

// Draws the mesh `source` (ARVX_MESH_WELDED, _SMOOTHED, _DECIMATED, _REFINED) that the model's context
// holds: the one the last marchingCubesMeshWelded / Smoothed / Decimated / Refined of this model built
// on the device, also after the model has moved on (renderWelded's note).  Only a missing welded mesh
// is built here, as renderWelded builds it; any other source that the context does not hold throws.
// source | ARVX_MESH_IMAGE_COLORS draws the mesh with the colours of the last colorMesh of that source
// (below), source | ARVX_MESH_TEXTURED with the atlas of the last textureMesh of that source; without
// that product the call throws.
inline RenderedView renderMesh(Model *model, int source, const float M[12], int W, int H,
                               const uint8_t *background = nullptr, const float *light = nullptr) {
    arvx_ctx *ctx = model->device_for_reading();
    const size_t stride = (size_t)(W > 0 ? W : 0) * 3;
    int rc = arvx_render_mesh(ctx, source, M, W, H, background, stride, light);
    if (rc == ARVX_ERR_STATE && source == ARVX_MESH_WELDED) {  // no welded mesh yet
        bool on_device = false;
        (void)model->inside_state(0.5f, on_device);
        if (on_device) {
            int apply_unseen = 0;
            ctx = detail::mesh_context(model, apply_unseen);
            int64_t nv = 0, nt = 0;
            detail::check(arvx_mc_mesh_welded(ctx, apply_unseen, &nv, &nt), "arvx_mc_mesh_welded");
            rc = arvx_render_mesh(ctx, source, M, W, H, background, stride, light);
        }
    }
    detail::check(rc, "arvx_render_mesh");
    return detail::rendered_view(ctx, W, H);
}

// The near plane of the model's triangle renders (arvx_ctx_set_render_near, defined in
// include/arvx/arvx.h): from the next renderMesh of either form on, faces that cross a2 = near are
// clipped against it in place of being refused, so a camera may stand inside the mesh.  0: none (the
// default).  The setting lives in the model's context: colorMesh, textureMesh and renderWelded ignore
// it.  An invalid value throws with the library's message.
inline void setRenderNear(Model *model, float near) {
    detail::check(arvx_ctx_set_render_near(model->device_for_reading(), near), "arvx_ctx_set_render_near");
}

inline float renderNear(Model *model) {
    float near = 0.f;
    detail::check(arvx_ctx_render_near(model->device_for_reading(), &near), "arvx_ctx_render_near");
    return near;
}

// What the near plane did to the faces of the model's current triangle render
// (arvx_render_mesh_clip_stats); zeros for a render made without a plane.
struct RenderClipStats {
    int64_t behind = 0, straddling = 0, pieces = 0, piecesDrawn = 0;
};

inline RenderClipStats renderMeshClipStats(Model *model) {
    int64_t out[4] = {0, 0, 0, 0};
    detail::check(arvx_render_mesh_clip_stats(model->device_for_reading(), out), "arvx_render_mesh_clip_stats");
    RenderClipStats st;
    st.behind = out[0], st.straddling = out[1], st.pieces = out[2], st.piecesDrawn = out[3];
    return st;
}

// ---- mesh colours from the images (an extension beyond the reference) -----------------------------
//
// The vertices of the mesh `source` that the model's context holds, coloured from the views' images
// (arvx_mesh_color, defined in include/arvx/arvx.h): per view the depth buffer of the mesh's own
// triangles, per vertex a vote -- mode ARVX_COLOR_CLOSEST or ARVX_COLOR_AVERAGE -- over the views that
// see it within `tolerance` (world units), sampled bilinearly; ARVX_MESH_COLOR_FOREGROUND in `flags`
// drops the views whose mask has the vertex's pixel as background.  The views are bound with their
// masks and their images.  renderMesh(model, source | ARVX_MESH_IMAGE_COLORS, ...) then draws the mesh
// with these colours, until the source mesh is built again.
struct MeshColors {
    std::vector<float> rgb;      // r, g, b per vertex
    std::vector<int32_t> views;  // the views that see each vertex
    int64_t coloured = 0;        // vertices some view sees
};

inline MeshColors colorMesh(const Intrinsics &intr, Model *model, const std::vector<View> &views, int source,
                            int mode, float tolerance, unsigned flags = 0) {
    arvx_ctx *ctx = detail::bind_views(intr, *model, views, false);
    model->set_colors_on_device(false);  // (arvx_set_views drops the context's colour list)
    std::vector<const uint8_t *> imgs(views.size());
    for (size_t i = 0; i < views.size(); ++i) {
        const Image &im = views[i].image;
        if (!im.data || im.channels != 3 || im.width != views[0].mask.width || im.height != views[0].mask.height ||
            im.stride != views[0].image.stride)
            throw Error(ARVX_ERR_INVALID, "colorMesh: colour images must be BGR u8 with the masks' size");
        imgs[i] = im.data;
    }
    detail::check(arvx_set_images(ctx, imgs.data(), views[0].image.stride), "arvx_set_images");
    MeshColors out;
    int rc = arvx_mesh_color(ctx, source, mode, tolerance, flags, &out.coloured);
    if (rc == ARVX_ERR_STATE && source == ARVX_MESH_WELDED) {  // no welded mesh yet: built as renderMesh builds it
        bool on_device = false;
        (void)model->inside_state(0.5f, on_device);
        if (on_device) {
            int apply_unseen = 0;
            ctx = detail::mesh_context(model, apply_unseen);
            int64_t nv = 0, nt = 0;
            detail::check(arvx_mc_mesh_welded(ctx, apply_unseen, &nv, &nt), "arvx_mc_mesh_welded");
            rc = arvx_mesh_color(ctx, source, mode, tolerance, flags, &out.coloured);
        }
    }
    detail::check(rc, "arvx_mesh_color");
    int64_t vertices = 0;
    detail::check(arvx_mesh_color_count(ctx, &vertices, nullptr), "arvx_mesh_color_count");
    out.rgb.resize(3 * (size_t)vertices);
    out.views.resize((size_t)vertices);
    detail::check(arvx_mesh_color_download(ctx, out.rgb.data(), out.views.data()), "arvx_mesh_color_download");
    return out;
}

// ---- mesh textures from the images (an extension beyond the reference) ----------------------------
//
// A texture atlas of the mesh `source` that the model's context holds (arvx_mesh_texture, defined in
// include/arvx/arvx.h): one triangle of texels per face, `resolution` texels along a leg, two faces per
// cell, `atlas_width` texels per atlas row; each face sampled from the view that sees its three corners
// within `tolerance` (world units) and shows it largest.  ARVX_MESH_TEXTURE_FOREGROUND in `flags` as
// ARVX_MESH_COLOR_FOREGROUND.  The views are bound with their masks and their images, as colorMesh
// binds them.  renderMesh(model, source | ARVX_MESH_TEXTURED, ...) then draws the mesh with the atlas,
// until the source mesh is built again; writeOBJ (include/arvx/mesh_texture.hpp) writes it.
inline MeshTexture textureMesh(const Intrinsics &intr, Model *model, const std::vector<View> &views, int source,
                               int resolution, int atlas_width = 4096, float tolerance = 0.f, unsigned flags = 0) {
    arvx_ctx *ctx = detail::bind_views(intr, *model, views, false);
    model->set_colors_on_device(false);  // (arvx_set_views drops the context's colour list)
    std::vector<const uint8_t *> imgs(views.size());
    for (size_t i = 0; i < views.size(); ++i) {
        const Image &im = views[i].image;
        if (!im.data || im.channels != 3 || im.width != views[0].mask.width || im.height != views[0].mask.height ||
            im.stride != views[0].image.stride)
            throw Error(ARVX_ERR_INVALID, "textureMesh: colour images must be BGR u8 with the masks' size");
        imgs[i] = im.data;
    }
    detail::check(arvx_set_images(ctx, imgs.data(), views[0].image.stride), "arvx_set_images");
    int64_t n[4] = {0, 0, 0, 0};
    int rc = arvx_mesh_texture(ctx, source, resolution, atlas_width, tolerance, flags, n);
    if (rc == ARVX_ERR_STATE && source == ARVX_MESH_WELDED) {  // no welded mesh yet: built as renderMesh builds it
        bool on_device = false;
        (void)model->inside_state(0.5f, on_device);
        if (on_device) {
            int apply_unseen = 0;
            ctx = detail::mesh_context(model, apply_unseen);
            int64_t nv = 0, nt = 0;
            detail::check(arvx_mc_mesh_welded(ctx, apply_unseen, &nv, &nt), "arvx_mc_mesh_welded");
            rc = arvx_mesh_texture(ctx, source, resolution, atlas_width, tolerance, flags, n);
        }
    }
    detail::check(rc, "arvx_mesh_texture");
    MeshTexture out;
    out.faces = n[0], out.textured = n[1];
    out.width = (int)n[2], out.height = (int)n[3], out.resolution = resolution;
    out.atlas.resize((size_t)n[2] * (size_t)n[3] * 3);
    out.face_view.resize((size_t)n[0]);
    out.face_uv.resize(6 * (size_t)n[0]);
    detail::check(arvx_mesh_texture_download(ctx, out.atlas.data(), out.face_view.data(), out.face_uv.data()),
                  "arvx_mesh_texture_download");
    return out;
}

// writeOBJ of a SimpleMesh: its vertices scaled and moved as WriteMesh scales and moves them.
inline bool writeOBJ(const std::string &path, const SimpleMesh &mesh, const MeshTexture &texture, float scaleFactor = 1.f,
                     Vec3f translation = Vec3f(0, 0, 0)) {
    const HostVector<Vec3f> &mv = mesh.GetVertices();
    const HostVector<Triangle> &mt = mesh.GetTriangles();
    std::vector<float> v(3 * mv.size());
    for (size_t i = 0; i < mv.size(); ++i) {
        volatile float px = mv[i].x() * scaleFactor, py = mv[i].y() * scaleFactor, pz = mv[i].z() * scaleFactor;
        v[3 * i] = px + translation.x(), v[3 * i + 1] = py + translation.y(), v[3 * i + 2] = pz + translation.z();
    }
    static_assert(sizeof(Triangle) == 24, "a face record: three indices, then r, g, b");
    return writeOBJ(path, v.data(), mv.size(), mt.empty() ? nullptr : &mt[0].idx0, mt.size(), 6, texture);
}

// Draws a mesh of the caller's on the model's context (arvx_render_triangles): its vertices in voxel
// units, as the marchingCubesMesh* calls return them.  vertex_rgb: 3 floats per vertex; null: every
// vertex takes the colour of the first triangle that contains it (black where there is none).
inline RenderedView renderMesh(Model *model, const SimpleMesh &mesh, const float M[12], int W, int H,
                               const uint8_t *background = nullptr, const float *light = nullptr,
                               const float *vertex_rgb = nullptr) {
    arvx_ctx *ctx = model->device_for_reading();
    const HostVector<Vec3f> &mv = mesh.GetVertices();
    const HostVector<Triangle> &mt = mesh.GetTriangles();
    std::vector<float> rgb;
    if (!vertex_rgb) {
        rgb.assign(3 * mv.size(), 0.f);
        for (size_t t = mt.size(); t-- > 0;) {  // (descending: the first triangle writes last)
            const unsigned corner[3] = {mt[t].idx0, mt[t].idx1, mt[t].idx2};
            for (unsigned i : corner) {
                if (i >= mv.size()) continue;  // (the call refuses the mesh)
                rgb[3 * (size_t)i] = (float)mt[t].r;
                rgb[3 * (size_t)i + 1] = (float)mt[t].g;
                rgb[3 * (size_t)i + 2] = (float)mt[t].b;
            }
        }
        vertex_rgb = rgb.data();
    }
    static_assert(sizeof(Triangle) == 24, "a face record: three indices, then r, g, b");
    detail::check(arvx_render_triangles(ctx, (int64_t)mv.size(), mv.empty() ? nullptr : mv[0].data(), vertex_rgb, (int64_t)mt.size(),
                                        mt.empty() ? nullptr : &mt[0].idx0, M, W, H, background,
                                        (size_t)(W > 0 ? W : 0) * 3, light),
                  "arvx_render_triangles");
    return detail::rendered_view(ctx, W, H);
}

// ---- relaxed mesh (an extension beyond the reference) ---------------------------------------------
//
// Taubin smoothing and vertex normals of the mesh `source` (ARVX_MESH_WELDED, _SMOOTHED, _DECIMATED,
// _REFINED) that the model's context holds (arvx_mesh_relax, defined in include/arvx/arvx.h): the mesh
// with the base's triangles and face colours and the relaxed vertices; normals, if not null, gets 3
// floats per vertex.  A source the context does not hold throws.  renderMesh, colorMesh and textureMesh
// then take ARVX_MESH_RELAXED as their source, until the base mesh is built again.
inline SimpleMesh relaxMesh(Model *model, int source, int iterations = 1, float lambda = 0.5f, float mu = -0.53f,
                            std::vector<float> *normals = nullptr) {
    arvx_ctx *ctx = model->device_for_reading();
    detail::check(arvx_mesh_relax(ctx, source, iterations, lambda, mu), "arvx_mesh_relax");
    int64_t n[3] = {0, 0, 0};
    detail::check(arvx_mesh_relax_info(ctx, n), "arvx_mesh_relax_info");
    SimpleMesh mesh;
    HostVector<Vec3f> &mv = mesh.GetVertices();
    HostVector<Triangle> &mt = mesh.GetTriangles();
    mv.resize((size_t)n[1]);  // (recycled memory, not zeroed: host_pool.hpp)
    mt.resize((size_t)n[2]);
    float *v = n[1] ? mv[0].data() : nullptr;
    uint32_t *f = n[2] ? &mt[0].idx0 : nullptr;
    static_assert(sizeof(Triangle) == 24, "a face record: three indices, then r, g, b");
    // (the base's download for its faces; its positions land where the relaxed ones follow)
    if (source == ARVX_MESH_DECIMATED)
        detail::check(arvx_mc_mesh_decimate_download(ctx, v, f, nullptr, nullptr, nullptr), "arvx_mc_mesh_decimate_download");
    else if (source == ARVX_MESH_REFINED)
        detail::check(arvx_mc_mesh_refined_download(ctx, v, f, nullptr, nullptr, nullptr), "arvx_mc_mesh_refined_download");
    else
        detail::check(arvx_mc_mesh_welded_download(ctx, v, f, nullptr), "arvx_mc_mesh_welded_download");
    if (normals) normals->resize(3 * (size_t)n[1]);
    detail::check(arvx_mesh_relax_download(ctx, v, normals && n[1] ? normals->data() : nullptr, nullptr),
                  "arvx_mesh_relax_download");
    return mesh;
}

// The same for a mesh of the caller's, relaxed on the model's context (arvx_mesh_relax_triangles): its
// vertices in any units within 2^20, as the marchingCubesMesh* calls return them.  The context's own
// relaxed mesh stays as it was.
inline SimpleMesh relaxMesh(Model *model, const SimpleMesh &mesh, int iterations = 1, float lambda = 0.5f,
                            float mu = -0.53f, std::vector<float> *normals = nullptr) {
    arvx_ctx *ctx = model->device_for_reading();
    SimpleMesh out = mesh;
    const HostVector<Vec3f> &mv = mesh.GetVertices();
    const HostVector<Triangle> &mt = mesh.GetTriangles();
    HostVector<Vec3f> &ov = out.GetVertices();
    if (normals) normals->resize(3 * mv.size());
    static_assert(sizeof(Triangle) == 24, "a face record: three indices, then r, g, b");
    detail::check(arvx_mesh_relax_triangles(ctx, (int64_t)mv.size(), mv.empty() ? nullptr : mv[0].data(),
                                            (int64_t)mt.size(), mt.empty() ? nullptr : &mt[0].idx0, iterations, lambda,
                                            mu, ov.empty() ? nullptr : ov[0].data(),
                                            normals && !mv.empty() ? normals->data() : nullptr, nullptr),
                  "arvx_mesh_relax_triangles");
    return out;
}

namespace detail {
// carve(..., intermediateMeshes = true) without a caller-supplied hook writes what the
// reference writes after every view (src/VoxelCarving.cpp:65-68): the model so far, moved
// along x by i * (X + 2) voxels.  (The directory is the caller's to create, as in the
// reference: src/main.cpp:47.)
inline bool install_default_intermediate_hook() {
    defaultIntermediateHook() = [](int i, Model &model) {
        marchingCubes(&model, 1.0f, Vec3f(i * (model.getX() + 2) * model.getSize(), 0, 0), 0.5f,
                      (std::string)("out/intermediate/image_" + std::to_string(i) + "_mesh.off"));
    };
    return true;
}
static const bool default_intermediate_hook_installed = install_default_intermediate_hook();
}  // namespace detail

}  // namespace arvx
#endif
