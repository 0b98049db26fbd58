// test_mesh_texture_host.cpp -- the atlas layout and the OBJ writer of include/arvx/mesh_texture.hpp on
// the host alone, and arvx::textureMesh, arvx::writeOBJ and arvx::renderMesh with ARVX_MESH_TEXTURED
// (include/arvx/marching_cubes.hpp) on a scene from a file, for tests/test_mesh_texture_cpp_gpu.py.
//
//   test_mesh_texture_host layout <dir>
//     no device: sweeps the layout (every texel owned by at most one face, the halves tile their cell,
//     owner() inverts texel(), the corners' UVs), writes a small textured mesh to <dir>/host.obj and reads
//     its three files back.  Prints "layout ok".  Built with -DARVX_MESH_TEXTURE_HOST_ONLY it is this mode
//     alone and needs no library.
//   test_mesh_texture_host <scene> <out> <obj> <bisections> <view> <R> <AW> <tolerance in voxel edges> <flags>
//     scene: tests/cpp/test_host.cpp's scene file (test_mesh_color_host.cpp describes it)
//     out:   int64 {T, textured, AW, AH}, the atlas, T ints of face_view, 6 T floats of face_uv, then one
//            render: W*H*3 bytes of bgr, W*H floats of depth, W*H ints of id
//     The model is carved with the scene's views, meshed by marchingCubesMeshRefined and textured by
//     textureMesh(ARVX_MESH_REFINED); <obj> is writeOBJ of that mesh; the render is
//     renderMesh(ARVX_MESH_REFINED | ARVX_MESH_TEXTURED) from view <view> over its image with a light at
//     the camera.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#ifdef ARVX_MESH_TEXTURE_HOST_ONLY
#include "arvx/mesh_texture.hpp"
#else
#include "arvx/marching_cubes.hpp"
#endif

namespace {

#define EXPECT(cond)                                                           \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);            \
            return false;                                                      \
        }                                                                      \
    } while (0)

bool layout_sweep() {
    const int resolutions[] = {1, 2, 3, 4, 5, 6, 7, 8, 37, 253};
    const int64_t counts[] = {0, 1, 2, 5, 8, 33};
    for (int R : resolutions)
        for (int64_t T : counts) {
            const int cw = R + 3, ch = R + 2;
            const int widths[] = {cw, 3 * cw, 3 * cw + 1, 5 * cw - 1};
            for (int AW : widths) {
                const arvx::MeshTextureLayout lay(T, R, AW);
                EXPECT(lay.valid() && lay.per_row == AW / cw);
                EXPECT(lay.AH == (int)(((T + 1) / 2 + lay.per_row - 1) / lay.per_row) * ch);
                std::vector<int64_t> owner((size_t)lay.AW * (size_t)lay.AH, -1);
                size_t owned = 0;
                for (int64_t f = 0; f < T; ++f)
                    for (int i = 0; i <= R + 1; ++i)
                        for (int j = 0; i + j <= R + 1; ++j) {
                            int x, y, oi = -1, oj = -1;
                            lay.texel(f, i, j, x, y);
                            EXPECT(x >= 0 && y >= 0 && x < lay.AW && y < lay.AH);
                            EXPECT(owner[(size_t)y * lay.AW + x] == -1);
                            owner[(size_t)y * lay.AW + x] = f;
                            ++owned;
                            EXPECT(lay.owner(x, y, oi, oj) == f && oi == i && oj == j);
                        }
                EXPECT(owned == (size_t)T * (size_t)((R + 2) * (R + 3) / 2));
                for (int y = 0; y < lay.AH; ++y)
                    for (int x = 0; x < lay.AW; ++x) {
                        int i, j;
                        EXPECT(lay.owner(x, y, i, j) == owner[(size_t)y * lay.AW + x]);
                    }
                for (int64_t k = 0; k < T / 2; ++k)  // the two halves tile their cell
                    for (int y = 0; y < ch; ++y)
                        for (int x = 0; x < cw; ++x) {
                            const int64_t o = owner[(size_t)((int)(k / lay.per_row) * ch + y) * lay.AW + (int)(k % lay.per_row) * cw + x];
                            EXPECT(o == 2 * k || o == 2 * k + 1);
                        }
                const std::vector<float> uv = lay.uv();
                EXPECT(uv.size() == 6 * (size_t)T);
                for (int64_t f = 0; f < T; ++f)
                    for (int k = 0; k < 3; ++k) {
                        int x, y;
                        lay.texel(f, k == 1 ? R : 0, k == 2 ? R : 0, x, y);
                        EXPECT(uv[6 * f + 2 * k] == ((float)x + 0.5f) / (float)AW);
                        EXPECT(uv[6 * f + 2 * k + 1] == ((float)y + 0.5f) / (float)lay.AH);
                    }
            }
        }
    EXPECT(!arvx::MeshTextureLayout(4, 0, 64).valid() && !arvx::MeshTextureLayout(4, 254, 4096).valid());
    EXPECT(!arvx::MeshTextureLayout(4, 2, 4).valid() && !arvx::MeshTextureLayout(4, 2, 16385).valid());
    EXPECT(!arvx::MeshTextureLayout(2000, 100, 103).valid());  // (1000 rows of 102 texels)
    return true;
}

bool writer_round_trip(const std::string &dir) {
    // a square of two faces and a third face on its own: T odd, an atlas with padding
    const float verts[] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.25f, 1.f, 1.f, 0.f, 0.f, 1.f, -3.5f, 2.f, 2.f, 1e-3f};
    const unsigned faces[] = {0, 1, 2, 9, 9, 9, 0, 2, 3, 9, 9, 9, 2, 4, 3, 9, 9, 9};
    const int R = 3;
    const arvx::MeshTextureLayout lay(3, R, 8);
    arvx::MeshTexture tex;
    tex.faces = 3, tex.textured = 2, tex.width = lay.AW, tex.height = lay.AH, tex.resolution = R;
    tex.atlas.resize((size_t)lay.AW * lay.AH * 3);
    for (size_t k = 0; k < tex.atlas.size(); ++k) tex.atlas[k] = (uint8_t)(37 * k + 11);
    tex.face_view = {0, 1, -1};
    tex.face_uv = lay.uv();
    const std::string path = dir + "/host.obj";
    EXPECT(arvx::writeOBJ(path, verts, 5, faces, 3, 6, tex));
    std::ifstream obj(path);
    std::string line;
    size_t nv = 0, nvt = 0, nf = 0;
    bool lib = false;
    while (std::getline(obj, line)) {
        std::istringstream in(line);
        std::string tag;
        in >> tag;
        if (tag == "mtllib") {
            std::string name;
            in >> name;
            lib = name == "host.mtl";
        } else if (tag == "v") {
            float x, y, z;
            EXPECT((bool)(in >> x >> y >> z));
            EXPECT(x == verts[3 * nv] && y == verts[3 * nv + 1] && z == verts[3 * nv + 2]);
            ++nv;
        } else if (tag == "vt") {
            float u, v;
            EXPECT((bool)(in >> u >> v));
            EXPECT(u == tex.face_uv[2 * nvt] && v == 1.0f - tex.face_uv[2 * nvt + 1]);
            ++nvt;
        } else if (tag == "f") {
            for (int k = 0; k < 3; ++k) {
                unsigned a = 0, ta = 0;
                char slash = 0;
                EXPECT((bool)(in >> a >> slash >> ta) && slash == '/');
                EXPECT(a == faces[6 * nf + k] + 1 && ta == 3 * nf + k + 1);
            }
            ++nf;
        }
    }
    EXPECT(lib && nv == 5 && nvt == 9 && nf == 3);
    std::ifstream mtl(dir + "/host.mtl");
    std::stringstream all;
    all << mtl.rdbuf();
    EXPECT(all.str().find("map_Kd host.ppm\n") != std::string::npos);
    std::ifstream ppm(dir + "/host.ppm", std::ios::binary);
    std::string magic;
    int w = 0, h = 0, top = 0;
    EXPECT((bool)(ppm >> magic >> w >> h >> top) && magic == "P6" && w == lay.AW && h == lay.AH && top == 255);
    ppm.get();
    std::vector<uint8_t> rgb(tex.atlas.size());
    ppm.read((char *)rgb.data(), (std::streamsize)rgb.size());
    EXPECT((bool)ppm && ppm.peek() == EOF);
    for (size_t p = 0; p < rgb.size(); p += 3)
        EXPECT(rgb[p] == tex.atlas[p + 2] && rgb[p + 1] == tex.atlas[p + 1] && rgb[p + 2] == tex.atlas[p]);
    tex.face_uv.pop_back();  // a texture that is not the mesh's is refused
    EXPECT(!arvx::writeOBJ(path, verts, 5, faces, 3, 6, tex));
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc >= 3 && std::strcmp(argv[1], "layout") == 0) {
        if (!layout_sweep() || !writer_round_trip(argv[2])) return 1;
        std::printf("layout ok\n");
        return 0;
    }
#ifdef ARVX_MESH_TEXTURE_HOST_ONLY
    std::fprintf(stderr, "usage: test_mesh_texture_host layout <dir>\n");
    return 2;
#else
    if (argc < 10) {
        std::fprintf(stderr, "usage: test_mesh_texture_host layout <dir> | <scene> <out> <obj> <bisections> <view> <R> "
                             "<AW> <tol> <flags>\n");
        return 2;
    }
    std::ifstream f(argv[1], std::ios::binary);
    int32_t hd[7] = {0, 0, 0, 0, 0, 0, 0};
    f.read((char *)hd, sizeof hd);
    const int X = hd[0], Y = hd[1], Z = hd[2], V = hd[3], W = hd[4], H = hd[5], C = hd[6];
    float s = 0.f;
    f.read((char *)&s, 4);
    arvx::Intrinsics intr;
    f.read((char *)intr.K, 36);
    std::vector<arvx::View> views((size_t)V);
    for (auto &v : views) f.read((char *)v.pose, 48);
    std::vector<uint8_t> masks((size_t)V * H * W * C), images((size_t)V * H * W * 3), st0((size_t)X * Y * Z);
    f.read((char *)masks.data(), (std::streamsize)masks.size());
    f.read((char *)images.data(), (std::streamsize)images.size());
    f.read((char *)st0.data(), (std::streamsize)st0.size());
    if (!f) {
        std::fprintf(stderr, "short scene file\n");
        return 2;
    }
    for (int i = 0; i < V; ++i) {
        views[(size_t)i].mask = {masks.data() + (size_t)i * H * W * C, W, H, C, (size_t)W * C};
        views[(size_t)i].image = {images.data() + (size_t)i * H * W * 3, W, H, 3, (size_t)W * 3};
    }
    const int bisections = std::atoi(argv[4]), view = std::atoi(argv[5]), R = std::atoi(argv[6]), AW = std::atoi(argv[7]);
    const float tolerance = (float)std::atof(argv[8]) * s;
    const unsigned flags = (unsigned)std::atoi(argv[9]);
    if (view < 0 || view >= V) return 2;
    try {
        arvx::Model model(X, Y, Z, s);
        arvx::carve(intr, model, views);
        float M[12];
        arvx::detail::check(arvx_compose_projection(intr.K, views[(size_t)view].pose, M), "arvx_compose_projection");
        const float light[3] = {M[9], M[8], -M[10]};
        const uint8_t *bg = images.data() + (size_t)view * H * W * 3;
        const int drawn = ARVX_MESH_REFINED | ARVX_MESH_TEXTURED;
        const arvx::SimpleMesh mesh = arvx::marchingCubesMeshRefined(intr, &model, views, bisections);
        bool threw = false;
        try {  // no texture yet
            (void)arvx::renderMesh(&model, drawn, M, W, H, bg, light);
        } catch (const arvx::Error &) {
            threw = true;
        }
        if (!threw) return 4;
        const arvx::MeshTexture tex = arvx::textureMesh(intr, &model, views, ARVX_MESH_REFINED, R, AW, tolerance, flags);
        if ((size_t)tex.faces != mesh.GetTriangles().size()) return 5;
        if (tex.face_uv != arvx::MeshTextureLayout(tex.faces, R, AW).uv()) return 6;  // (the host's layout is the library's)
        if (!arvx::writeOBJ(argv[3], mesh, tex, s)) return 7;
        const arvx::RenderedView r = arvx::renderMesh(&model, drawn, M, W, H, bg, light);
        std::ofstream o(argv[2], std::ios::binary);
        const int64_t head[4] = {tex.faces, tex.textured, tex.width, tex.height};
        o.write((const char *)head, sizeof head);
        o.write((const char *)tex.atlas.data(), (std::streamsize)tex.atlas.size());
        o.write((const char *)tex.face_view.data(), (std::streamsize)(tex.face_view.size() * sizeof(int32_t)));
        o.write((const char *)tex.face_uv.data(), (std::streamsize)(tex.face_uv.size() * sizeof(float)));
        o.write((const char *)r.bgr.data(), (std::streamsize)r.bgr.size());
        o.write((const char *)r.depth.data(), (std::streamsize)(r.depth.size() * sizeof(float)));
        o.write((const char *)r.id.data(), (std::streamsize)(r.id.size() * sizeof(int32_t)));
        if (!o) return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
    return 0;
#endif
}
