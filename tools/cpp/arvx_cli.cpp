// arvx_cli.cpp -- the reference's command line (src/main.cpp:16-39) for the parts of it that
// this library covers: `-c=5` (voxel carving: carve | fastCarve -> colour -> handleUnseen ->
// [closure] -> marching cubes -> OFF file, src/main.cpp:184-305) and `-c=6` (the eight-run
// benchmark table, :306-440), with the reference's flag names, defaults, checks, messages
// and stage order.
//
// What the reference does with OpenCV before its voxel loops -- JPEG decoding, ChArUco pose
// estimation, cv::undistort -- is not in this image, so the inputs are what those
// steps produce:
//   -images=<dir> -masks=<dir>   binary PPM (P6) / PGM (P5) files, already undistorted, taken
//                                in sorted file-name order like cv::glob
//   -poses=<file>                one world->camera matrix per view, 12 floats per line: the
//                                top three rows of estimatePoseFromImage(...).inv()
//                                (src/VoxelCarving.cpp:25-26)
//   -scene=<file>                or all of it in one binary file (tests/cpp/test_host.cpp)
//   -segment=range|plate         the masks from the images, on the device (arvx_segment_views):
//                                -masks is then not needed
//   -calibration=<yml>           the reference's calibration file; its camera matrix is used
//                                (src/PoseEstimation.h:11-16), the distortion coefficients only
//                                with -undistort=true: then the inputs are RAW images and
//                                arvx_undistort remaps them on the device (see arvx.h)
// -c=1..4 (board creation, camera calibration, live pose estimation, segmentation) are
// OpenCV/aruco programs around the path and are not provided; the range rule of -c=4
// (src/Segmentation.h:10-11) runs inside -c=5 / -c=6 as -segment=range.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "arvx/calibration.hpp"
#include "arvx/segmentation.hpp"
#include "bench6.hpp"

namespace fs = std::filesystem;

namespace {

const char *about = "AR Voxel Carving Project\n";

// cv::CommandLineParser-like: -name=value or --name=value; a bare -name means true
struct Args {
    std::map<std::string, std::string> kv;
    Args(int argc, char **argv, const std::map<std::string, std::string> &defaults) : kv(defaults) {
        for (int i = 1; i < argc; ++i) {
            std::string a = argv[i];
            while (!a.empty() && a[0] == '-') a.erase(0, 1);
            const size_t eq = a.find('=');
            if (eq == std::string::npos) kv[a] = "true";
            else kv[a.substr(0, eq)] = a.substr(eq + 1);
        }
    }
    std::string str(const std::string &k) const {
        auto it = kv.find(k);
        return it == kv.end() ? "" : it->second;
    }
    int i(const std::string &k) const { return std::atoi(str(k).c_str()); }
    float f(const std::string &k) const { return (float)std::atof(str(k).c_str()); }
    bool b(const std::string &k) const {
        const std::string v = str(k);
        return v == "true" || v == "1" || v == "TRUE" || v == "True";
    }
};

struct Picture {
    int w = 0, h = 0, c = 0;
    std::vector<uint8_t> px;
};

// binary PGM (P5, 1 channel) / PPM (P6, RGB -> stored BGR like cv::imread)
bool read_pnm(const std::string &path, Picture &out, bool as_color) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::string magic;
    f >> magic;
    if (magic != "P5" && magic != "P6") return false;
    auto next_int = [&]() {
        int v = 0;
        for (;;) {
            int ch = f.peek();
            if (ch == '#') {
                std::string line;
                std::getline(f, line);
            } else if (isspace(ch)) {
                f.get();
            } else {
                break;
            }
        }
        f >> v;
        return v;
    };
    const int w = next_int(), h = next_int(), maxv = next_int();
    f.get();  // the single whitespace before the raster
    if (w < 1 || h < 1 || maxv != 255) return false;
    const int cin = magic == "P6" ? 3 : 1;
    std::vector<uint8_t> raw((size_t)w * h * cin);
    f.read((char *)raw.data(), (std::streamsize)raw.size());
    if (!f) return false;
    out.w = w;
    out.h = h;
    out.c = as_color ? 3 : cin;  // cv::imread(.., 1): always 3 channels, BGR
    out.px.resize((size_t)w * h * out.c);
    for (size_t p = 0; p < (size_t)w * h; ++p) {
        if (cin == 3 && out.c == 3) {
            out.px[3 * p] = raw[3 * p + 2];
            out.px[3 * p + 1] = raw[3 * p + 1];
            out.px[3 * p + 2] = raw[3 * p];
        } else if (cin == 1 && out.c == 3) {
            out.px[3 * p] = out.px[3 * p + 1] = out.px[3 * p + 2] = raw[p];
        } else {
            out.px[p] = raw[p];
        }
    }
    return true;
}

std::vector<std::string> glob_sorted(const std::string &dir) {  // cv::glob: sorted names
    std::vector<std::string> names;
    if (!fs::is_directory(dir)) return names;
    for (const auto &e : fs::directory_iterator(dir))
        if (e.is_regular_file()) names.push_back(e.path().string());
    std::sort(names.begin(), names.end());
    return names;
}

struct Inputs {
    arvx::Intrinsics intr{};
    std::vector<double> dist;
    std::vector<arvx::View> views;
    std::vector<Picture> images, masks;
    std::vector<uint8_t> scene_masks, scene_images;
};

// -scene=<file>: int32 X,Y,Z,V,W,H,C ; float s ; float K[9] ; V x pose[12] ; masks ; images
bool load_scene(const std::string &path, Inputs &in) {
    std::ifstream f(path, std::ios::binary);
    int32_t hd[7];
    f.read((char *)hd, sizeof hd);
    const int V = hd[3], W = hd[4], H = hd[5], C = hd[6];
    float s_unused;
    f.read((char *)&s_unused, 4);
    f.read((char *)in.intr.K, 36);
    if (!f || V < 1) return false;
    in.views.resize(V);
    for (auto &v : in.views) f.read((char *)v.pose, 48);
    in.scene_masks.resize((size_t)V * H * W * C);
    in.scene_images.resize((size_t)V * H * W * 3);
    f.read((char *)in.scene_masks.data(), (std::streamsize)in.scene_masks.size());
    f.read((char *)in.scene_images.data(), (std::streamsize)in.scene_images.size());
    if (!f) return false;
    for (int i = 0; i < V; ++i) {
        in.views[i].mask = {in.scene_masks.data() + (size_t)i * H * W * C, W, H, C, (size_t)W * C};
        in.views[i].image = {in.scene_images.data() + (size_t)i * H * W * 3, W, H, 3, (size_t)W * 3};
    }
    return true;
}

bool load_poses(const std::string &path, std::vector<arvx::View> &views) {
    std::ifstream f(path);
    if (!f) return false;
    for (auto &v : views)
        for (int k = 0; k < 12; ++k)
            if (!(f >> v.pose[k])) return false;
    return true;
}

// -render=DIR: DIR/render%04d.ppm per view, and one line per view with the agreement counts.
// mesh_source < 0: the welded mesh's vertex voxels (arvx_render); else, -renderMesh=true: the triangles
// of that mesh of the context (ARVX_MESH_*), shaded by a light at the camera (arvx_render_mesh).
bool render_views(const std::string &dir, const Inputs &in, arvx::Model &model, int mesh_source) {
    fs::create_directories(dir);
    const int V = (int)in.views.size();
    std::vector<uint8_t> bg, rgb;
    for (int i = 0; i < V; ++i) {
        const arvx::View &v = in.views[i];
        float M[12];
        if (v.has_M)
            std::memcpy(M, v.M, sizeof M);
        else
            arvx::detail::check(arvx_compose_projection(in.intr.K, v.pose, M), "arvx_compose_projection");
        const arvx::Image &im = v.image.data ? v.image : v.mask;
        const int W = im.width, H = im.height;
        const bool over = v.image.data && v.image.channels == 3;
        if (over) {  // (tightly packed rows)
            bg.resize((size_t)W * H * 3);
            for (int r = 0; r < H; ++r)
                std::memcpy(bg.data() + (size_t)r * W * 3, im.data + (size_t)r * im.stride, (size_t)W * 3);
        }
        const float light[3] = {M[9], M[8], -M[10]};  // the viewing direction along the voxel axes
        const arvx::RenderedView out =
            mesh_source < 0 ? arvx::renderWelded(&model, M, W, H, over ? bg.data() : nullptr)
                            : arvx::renderMesh(&model, mesh_source, M, W, H, over ? bg.data() : nullptr, light);
        if (mesh_source >= 0 && arvx::renderNear(&model) > 0.f) {  // -near=D: what the plane did to the faces
            const arvx::RenderClipStats st = arvx::renderMeshClipStats(&model);
            std::cout << "LOG - RENDER CLIP: view " << i << " behind " << st.behind << " straddling " << st.straddling
                      << " pieces " << st.pieces << " drawn " << st.piecesDrawn << std::endl;
        }
        rgb.resize(out.bgr.size());
        for (size_t p = 0; p < out.bgr.size(); p += 3) {
            rgb[p] = out.bgr[p + 2];
            rgb[p + 1] = out.bgr[p + 1];
            rgb[p + 2] = out.bgr[p];
        }
        char name[32];
        std::snprintf(name, sizeof name, "render%04d.ppm", i);
        std::ofstream f((fs::path(dir) / name).string(), std::ios::binary);
        f << "P6\n" << W << " " << H << "\n255\n";
        f.write((const char *)rgb.data(), (std::streamsize)rgb.size());
        if (!f) {
            std::cerr << "Could not write " << name << " (--render)" << std::endl;
            return false;
        }
    }
    // the masks again (the colour pass took the cameras only); the context's colour list goes
    arvx_ctx *ctx = arvx::detail::bind_views(in.intr, model, in.views, false);
    model.set_colors_on_device(false);
    for (int i = 0; i < V; ++i) {
        int64_t n[3];
        if (mesh_source < 0)
            arvx::detail::check(arvx_render_agreement(ctx, i, n), "arvx_render_agreement");
        else
            arvx::detail::check(arvx_render_mesh_agreement(ctx, mesh_source, i, n), "arvx_render_mesh_agreement");
        std::cout << (mesh_source < 0 ? "LOG - RENDER: view " : "LOG - RENDER MESH: view ") << i << " both " << n[0] << " model_only " << n[1] << " mask_only "
                  << n[2] << std::endl;
    }
    return true;
}

// the vertices and the faces' indices of an OFF file as SimpleMesh::WriteMesh writes it
bool read_off(const std::string &path, std::vector<float> &verts, std::vector<unsigned> &faces) {
    std::ifstream f(path);
    std::string magic;
    size_t nv = 0, nt = 0, ne = 0;
    if (!(f >> magic >> nv >> nt >> ne) || magic != "OFF") return false;
    verts.resize(3 * nv);
    for (float &c : verts) f >> c;
    faces.resize(3 * nt);
    for (size_t t = 0; t < nt; ++t) {
        unsigned n = 0, r, g, b;
        f >> n >> faces[3 * t] >> faces[3 * t + 1] >> faces[3 * t + 2] >> r >> g >> b;
        if (n != 3) return false;
    }
    return (bool)f;
}

}  // namespace

int main(int argc, char *argv[]) {
    // src/main.cpp:45-47
    fs::create_directories("./out");
    fs::create_directories("./out/tmp");
    fs::create_directories("./out/intermediate");
    const std::map<std::string, std::string> defaults = {
        {"calibration", "out/cameracalibration.yml"}, {"carve", "1"}, {"x", "100"}, {"y", "100"},
        {"z", "100"}, {"size", "0.0028"}, {"color", "0"}, {"scale", "1.0"}, {"dx", "0.0"},
        {"dy", "0.0"}, {"dz", "0.0"}, {"model_debug", "false"}, {"postprocessing", "true"},
        {"intermediateMesh", "false"}, {"outFile", "./out/mesh.off"}, {"undistort", "false"}, {"weld", "false"},
        {"smooth", "0"}, {"decimate", "0"}, {"visible", "false"}, {"visibleTol", "3"}, {"photo", "0"}, {"photoViews", "2"},
        {"photoIters", "32"}, {"render", ""}, {"misses", "0"}, {"floaters", "0"}, {"largest", "false"},
        {"erode", ""}, {"dilate", ""}, {"open", ""}, {"close", ""}, {"refine", ""}, {"relax", ""}, {"renderMesh", "false"}, {"near", "0"},
        {"meshColor", ""}, {"meshForeground", "false"}, {"texture", "0"}, {"atlasWidth", "4096"},
        {"segment", ""}, {"segLo", "120,120,120"}, {"segHi", "255,255,255"}, {"plates", ""}, {"segThreshold", "30"},
        {"segOpen", "0"}, {"segClose", "0"}, {"segMinArea", "0"}, {"segLargest", "false"}, {"segMaxHole", "0"},
        {"writeMasks", ""}};
    Args parser(argc, argv, defaults);
    if (argc < 2) {
        std::cout << about
                  << "  -c=5 voxel carving, -c=6 benchmark; -images -masks -poses | -scene, "
                     "-calibration, -carve, -x -y -z -size, -color, -scale -dx -dy -dz,\n"
                     "  -postprocessing, -intermediateMesh, -outFile (flags of the reference's "
                     "src/main.cpp:16-39), -weld (shared mesh vertices),\n"
                     "  -smooth=N (the welded mesh after N Taubin iterations, lambda 0.5, mu -0.53),\n"
                     "  -decimate=C (the welded mesh -- after -smooth=N, if given -- with the vertices of\n"
                     "    every cube of C^3 voxels merged into one, 1 <= C <= 64; 0, the default: off),\n"
                     "  -refine=B (in place of the plain mesh: one vertex per cut edge, placed where the edge\n"
                     "    leaves the masks' visual hull by B bisection steps, 0 <= B <= 10; 0: edge midpoints;\n"
                     "    not together with -smooth or -decimate),\n"
                     "  -relax=N (the mesh the run would write -- refined, decimated, smoothed, else welded --\n"
                     "    after N Taubin iterations, lambda 0.5, mu -0.53, on whatever mesh that is; -renderMesh,\n"
                     "    -meshColor and -texture then use the relaxed mesh),\n"
                     "  -visible=true (-color=1|2 over the views in which each voxel is visible),\n"
                     "  -visibleTol=T (its depth tolerance in voxel edges, default 3),\n"
                     "  -misses=K (-carve=1: empty a voxel only when more than K views see it as\n"
                     "    background; 0, the default: the reference's carve; K > 0 writes no\n"
                     "    intermediate meshes),\n"
                     "  -photo=T (after carving: remove surface voxels whose visible views' colours\n"
                     "    differ by a summed channel standard deviation above T; 0, the default: off),\n"
                     "  -photoViews=N (views a voxel must be visible in to be judged, default 2),\n"
                     "  -photoIters=N (sweeps at most, default 32; depth tolerance: -visibleTol),\n"
                     "  -floaters=N (after carving: empty every connected component of fewer than N\n"
                     "    voxels, 6-connectivity; 0, the default: off),\n"
                     "  -largest=true (after carving: keep only the largest connected component),\n"
                     "  -erode=R | -dilate=R | -open=R | -close=R (after carving and -photo, before\n"
                     "    -floaters / -largest: erosion, dilation, opening or closing of the model by a\n"
                     "    ball of radius R voxels, R >= 0 a float; at most one of them; an opening removes\n"
                     "    what is thinner than the ball, and -largest=true then drops what it cut loose),\n"
                     "  -render=DIR (after the mesh: the welded model drawn over every input image,\n"
                     "    DIR/renderNNNN.ppm, and its agreement with every mask),\n"
                     "  -renderMesh=true (with -render: the triangles of the mesh the run wrote -- refined,\n"
                     "    decimated, smoothed, else welded -- with a depth buffer and a light at the camera,\n"
                     "    in place of the welded model's voxels),\n"
                     "  -near=D (with -render and -renderMesh=true: faces that cross the plane at depth D in front of\n"
                     "    a camera are clipped against it, not refused, so a camera may stand inside the mesh;\n"
                     "    0, the default: off),\n"
                     "  -meshColor=closest|average (with -render and -renderMesh=true: the mesh's vertices\n"
                     "    coloured from the input images -- per view the depth buffer of the mesh itself, per\n"
                     "    vertex a vote over the views that see it within -visibleTol voxel edges, sampled\n"
                     "    bilinearly -- and the renders drawn with those colours),\n"
                     "  -meshForeground=true (with -meshColor: a view votes only where its mask has the\n"
                     "    vertex's pixel as foreground),\n"
                     "  -texture=R (the mesh the run wrote after -weld, -smooth, -decimate or -refine, textured\n"
                     "    from the input images: a triangle of texels per face, R texels along a leg, 1 <= R <=\n"
                     "    253, each face sampled from the view that sees its corners within -visibleTol voxel\n"
                     "    edges and shows it largest; written beside -outFile as <stem>.obj, .mtl and .ppm;\n"
                     "    with -render and -renderMesh=true the renders draw the texture; -meshForeground applies;\n"
                     "    not together with -meshColor),\n"
                     "  -atlasWidth=AW (texels per row of the texture atlas, default 4096),\n"
                     "  -segment=range|plate (the masks from the images, on the device; -masks is not needed:\n"
                     "    range: background where -segLo=B,G,R <= pixel <= -segHi=B,G,R, defaults 120,120,120 and\n"
                     "    255,255,255, the reference's -c=4; plate: foreground where a channel differs by more than\n"
                     "    -segThreshold=T, default 30, from the plate in -plates=<dir>, one file or one per image),\n"
                     "  -segOpen=R -segClose=R (the masks opened, then closed, by squares of side 2 R + 1),\n"
                     "  -segMinArea=N (foreground components of fewer than N pixels go, 8-connectivity),\n"
                     "  -segLargest=true (only the largest foreground component stays),\n"
                     "  -segMaxHole=N (enclosed background of at most N pixels is filled; -1: of any size),\n"
                     "  -writeMasks=DIR (with -segment: the final masks as DIR/maskNNNN.pgm)\n";
        return 0;
    }
    const int choose = parser.i("c");
    if (choose != 5 && choose != 6) {
        std::cerr << "-c=" << choose
                  << ": board creation, camera calibration, pose estimation and segmentation are "
                     "OpenCV/aruco programs of the reference and not part of this library (use "
                     "-c=5 or -c=6)"
                  << std::endl;
        return 1;
    }
    const char *tag = choose == 5 ? "VC" : "Benchmark";
    if (choose == 5) {
        const int carveArg = parser.i("carve");
        if (carveArg < 1 || 2 < carveArg) {
            std::cerr << "Invalid carve argument.";
            return 1;
        }
        if (parser.i("misses") < 0 || 65535 < parser.i("misses")) {
            std::cerr << "Invalid misses argument.";
            return 1;
        }
        if (parser.i("floaters") < 0) {
            std::cerr << "Invalid floaters argument.";
            return 1;
        }
        int morphs = 0;
        for (const char *name : {"erode", "dilate", "open", "close"}) {
            if (parser.str(name).empty()) continue;
            ++morphs;
            const float r = parser.f(name);
            if (!(r >= 0.f) || !(r < 46341.f)) {
                std::cerr << "Invalid " << name << " argument.";
                return 1;
            }
        }
        if (morphs > 1) {
            std::cerr << "At most one of -erode, -dilate, -open and -close may be given.";
            return 1;
        }
        if (!parser.str("relax").empty() && parser.i("relax") < 0) {
            std::cerr << "Invalid relax argument.";
            return 1;
        }
        if (!parser.str("refine").empty()) {
            if (parser.i("refine") < 0 || 10 < parser.i("refine")) {
                std::cerr << "Invalid refine argument.";
                return 1;
            }
            if (parser.i("smooth") > 0 || parser.i("decimate") > 0) {
                std::cerr << "-refine writes a mesh of its own: it cannot be combined with -smooth or -decimate.";
                return 1;
            }
        }
    }
    Inputs in;
    if (!parser.str("scene").empty()) {
        if (!load_scene(parser.str("scene"), in)) {
            std::cerr << "Could not read the scene file (--scene)" << std::endl;
            return 1;
        }
        std::cout << "LOG - " << tag << ": images read." << std::endl;
        std::cout << "LOG - " << tag << ": masks read." << std::endl;
    } else {
        const std::string image_dir = parser.str("images");
        if (image_dir.empty()) {
            std::cerr << "You need to define a images path (--images)" << std::endl;
            return 1;
        }
        if (choose == 5 && parser.f("scale") == 0)
            std::cerr << "The program won't compute stuff for fun! Enter a scale != 0.0" << std::endl;
        for (const std::string &name : glob_sorted(image_dir)) {
            Picture p;
            if (read_pnm(name, p, true)) in.images.push_back(std::move(p));
        }
        std::cout << "LOG - " << tag << ": images read." << std::endl;
        const std::string masks_dir = parser.str("masks");
        if (masks_dir.empty() && !parser.str("segment").empty()) {
            // -segment: the masks come from the images (below)
            if (in.images.empty()) {
                std::cerr << "No readable PPM/PGM files in --images" << std::endl;
                return 1;
            }
            in.masks.resize(in.images.size());
        } else if (masks_dir.empty()) {
            std::cerr << "You need to define a image masks path (--masks)" << std::endl;
            return 1;
        }
        if (!masks_dir.empty())
            for (const std::string &name : glob_sorted(masks_dir)) {
                Picture p;
                if (read_pnm(name, p, true)) in.masks.push_back(std::move(p));
            }
        std::cout << "LOG - " << tag << ": masks read." << std::endl;
        if (in.images.size() != in.masks.size()) {
            std::cerr << "Number of images doesn't match number of masks." << std::endl;
            return 1;
        }
        if (in.images.empty()) {
            std::cerr << "No readable PPM/PGM files in --images" << std::endl;
            return 1;
        }
        in.views.resize(in.images.size());
        for (size_t i = 0; i < in.views.size(); ++i) {
            const Picture &im = in.images[i], &mk = in.masks[i];
            in.views[i].image = {im.px.data(), im.w, im.h, im.c, (size_t)im.w * im.c};
            in.views[i].mask = {mk.px.data(), mk.w, mk.h, mk.c, (size_t)mk.w * mk.c};
        }
        if (parser.str("poses").empty() || !load_poses(parser.str("poses"), in.views)) {
            std::cerr << "You need to give the world->camera matrices of the views (--poses: 12 "
                         "floats per view); pose estimation itself is OpenCV-aruco"
                      << std::endl;
            return 1;
        }
    }
    int x = 0, y = 0, z = 0;
    float size = 0;
    if (choose == 5) {
        x = parser.i("x");
        y = parser.i("y");
        z = parser.i("z");
        if (x < 1 || y < 1 || z < 1) {
            std::cerr << "You need to define a valid number of voxels for the model. (--x/--y/--z)";
            return 1;
        }
        size = parser.f("size");
        if (size <= 0) {
            std::cerr << "You need to define a strictly positive voxel size. (--size)";
            return 1;
        }
    }
    if (parser.str("calibration").empty()) {
        std::cerr << "You need to define the path to the calibration file (--calibration)"
                  << std::endl;
        return 1;
    }
    double K[9];
    if (arvx::readCameraParameters(parser.str("calibration"), K, in.dist)) {
        for (int k = 0; k < 9; ++k) in.intr.K[k] = (float)K[k];  // convertTo(CV_32F), :29-30
    } else if (parser.str("scene").empty()) {
        std::cerr << "Invalid camera file" << std::endl;  // src/PoseEstimation.h:13
        return 1;
    }
    std::cout << "LOG - " << tag << ": read cameraMatrix and distCoefficients." << std::endl;
    if (parser.b("undistort")) {
        // raw inputs: what the reference does per view inside carve / the colour pass
        // (cv::undistort of mask and image, src/VoxelCarving.cpp:35-36), once, on the device
        arvx_ctx *u = nullptr;
        if (arvx_ctx_create(&u, 0, 8, 8, 8, 1.f) != ARVX_OK) return 3;
        const int V = (int)in.views.size();
        std::vector<const uint8_t *> src(V);
        std::vector<uint8_t *> dst(V);
        int rc = ARVX_OK;
        for (int pass = 0; pass < 2 && rc == ARVX_OK; ++pass) {
            for (int i = 0; i < V; ++i) {
                const arvx::Image &im = pass ? in.views[i].image : in.views[i].mask;
                src[i] = im.data;
                dst[i] = const_cast<uint8_t *>(im.data);
            }
            const arvx::Image &f = pass ? in.views[0].image : in.views[0].mask;
            if (!f.data) continue;
            rc = arvx_undistort(u, V, src.data(), f.width, f.height, f.channels, f.stride, K,
                                in.dist.data(), (int)in.dist.size(), dst.data());
        }
        arvx_ctx_destroy(u);
        if (rc != ARVX_OK) {
            std::cerr << "arvx_undistort: " << arvx_last_error() << std::endl;
            return 3;
        }
        std::cout << "LOG - " << tag << ": undistorted masks and images." << std::endl;
    }
    const arvx::Vec3f modelTranslation(parser.f("dx"), parser.f("dy"), parser.f("dz"));
    // -segment (an extension beyond the reference's -c=4): the masks from the images, on the device
    arvx::SegmentedMasks segmented;
    std::vector<Picture> plate_pictures;
    const auto segment = [&](arvx::Model &m) {
        const std::string kind = parser.str("segment");
        if (kind.empty()) return true;
        arvx::SegmentParams sp;
        if (kind == "plate") sp.rule = ARVX_SEGMENT_PLATE;
        else if (kind != "range") {
            std::cerr << "Invalid segment argument (range or plate)." << std::endl;
            return false;
        }
        int lo[3], hi[3];
        if (std::sscanf(parser.str("segLo").c_str(), "%d,%d,%d", lo, lo + 1, lo + 2) != 3 ||
            std::sscanf(parser.str("segHi").c_str(), "%d,%d,%d", hi, hi + 1, hi + 2) != 3) {
            std::cerr << "Invalid segLo / segHi argument (B,G,R)." << std::endl;
            return false;
        }
        for (int c = 0; c < 3; ++c) {
            if (lo[c] < 0 || hi[c] > 255 || lo[c] > hi[c]) {
                std::cerr << "Invalid segLo / segHi argument (0 <= lo <= hi <= 255)." << std::endl;
                return false;
            }
            sp.lo[c] = (uint8_t)lo[c];
            sp.hi[c] = (uint8_t)hi[c];
        }
        sp.threshold = parser.i("segThreshold");
        sp.open_radius = parser.i("segOpen");
        sp.close_radius = parser.i("segClose");
        sp.min_area = parser.i("segMinArea");
        sp.max_hole = parser.i("segMaxHole");
        sp.flags = parser.b("segLargest") ? ARVX_SEGMENT_LARGEST : 0u;
        std::vector<arvx::Image> plates;
        if (sp.rule == ARVX_SEGMENT_PLATE) {
            for (const std::string &name : glob_sorted(parser.str("plates"))) {
                Picture p;
                if (read_pnm(name, p, true)) plate_pictures.push_back(std::move(p));
            }
            if (plate_pictures.empty()) {
                std::cerr << "You need to define a background plates path (--plates)" << std::endl;
                return false;
            }
            for (const Picture &p : plate_pictures) plates.push_back({p.px.data(), p.w, p.h, p.c, (size_t)p.w * p.c});
        }
        arvx::segmentViews(m, in.views, sp, plates, segmented);
        for (size_t i = 0; i < segmented.counts.size(); ++i) {
            const auto &n = segmented.counts[i];
            std::cout << "LOG - SEG: view " << i << " foreground " << n[0] << " cleaned " << n[1] << " specks " << n[2]
                      << " holes " << n[3] << " (specks removed " << n[4] << ", " << n[5] << " px; holes filled "
                      << n[6] << ", " << n[7] << " px)" << std::endl;
        }
        const std::string dir = parser.str("writeMasks");
        if (!dir.empty()) {
            fs::create_directories(dir);
            for (size_t i = 0; i < segmented.masks.size(); ++i) {
                char name[32];
                std::snprintf(name, sizeof name, "mask%04d.pgm", (int)i);
                std::ofstream f((fs::path(dir) / name).string(), std::ios::binary);
                f << "P5\n" << segmented.width << " " << segmented.height << "\n255\n";
                f.write((const char *)segmented.masks[i].data(), (std::streamsize)segmented.masks[i].size());
                if (!f) {
                    std::cerr << "Could not write " << name << " (--writeMasks)" << std::endl;
                    return false;
                }
            }
        }
        std::cout << "LOG - SEG: masks segmented." << std::endl;
        return true;
    };
    try {
        if (choose == 6) {
            if (!parser.str("segment").empty()) {
                arvx::Model scratch(8, 8, 8, 1.f);  // (a context to segment on: the table makes its own models)
                if (!segment(scratch)) return 1;
            }
            bench6::run(in.intr, in.views, parser.f("scale"), modelTranslation);
            return 0;
        }
        // 100, 100, 100, 0.0028 ~ Caruco
        arvx::Model model(x, y, z, size);
        if (!segment(model)) return 1;
        switch (parser.i("carve")) {
            case 1:
                // -misses=K (an extension beyond the reference): the vote carve in place of carve()
                if (parser.i("misses") > 0)
                    arvx::carveVotes(in.intr, model, in.views, parser.i("misses"));
                else
                    arvx::carve(in.intr, model, in.views, parser.b("intermediateMesh"));
                break;
            case 2: arvx::fastCarve(in.intr, model, in.views); break;
        }
        // -photo (an extension beyond the reference): photo-consistency carving before the colours
        if (parser.f("photo") > 0.f)
            arvx::photoCarve(in.intr, model, in.views, parser.f("photo"), parser.i("photoViews"),
                             parser.f("visibleTol"), parser.i("photoIters"));
        // -erode=R, -dilate=R, -open=R, -close=R (an extension beyond the reference): ball morphology of
        // the carved model, before the components so that what an opening cuts loose can be dropped
        {
            const char *const names[] = {"erode", "dilate", "open", "close"};  // (ARVX_MORPH_* order)
            for (int op = 0; op < 4; ++op)
                if (!parser.str(names[op]).empty()) arvx::morph(model, op, parser.f(names[op]));
        }
        // -floaters=N, -largest=true (an extension beyond the reference): the model's connected
        // components -- the clumps that false foreground specks leave in mid-air go before they are coloured
        if (parser.i("floaters") > 0 || parser.b("largest"))
            arvx::dropFloaters(model, std::max(1, parser.i("floaters")), parser.b("largest"));
        const int color = parser.i("color");
        if (color < 0 || 3 < color) {
            std::cerr << "You need to select a predefined color reconstruction mode. (--color)";
            return 1;
        }
        // -visible (an extension beyond the reference): the vote over the views in which each
        // voxel is visible, depth tolerance -visibleTol voxel edges
        const bool visible = parser.b("visible");
        const float tol = parser.f("visibleTol");
        switch (color) {
            case 0: break;
            case 1:
                if (visible)
                    arvx::reconstructClosestColorVisible(in.intr, model, in.views, tol);
                else
                    arvx::reconstructClosestColor(in.intr, model, in.views);
                break;
            case 2:
                if (visible)
                    arvx::reconstructAvgColorVisible(in.intr, model, in.views, tol);
                else
                    arvx::reconstructAvgColor(in.intr, model, in.views);
                break;
            default: std::cerr << "Ups, something went wrong!" << std::endl;
        }
        model.handleUnseen();
        if (parser.b("model_debug"))
            std::cerr << "-model_debug: the reference's debug cube mesh (Model::WriteModel) is not "
                         "part of this library"
                      << std::endl;
        if (parser.b("postprocessing")) arvx::applyClosure(&model, 3);
        // -weld (an extension beyond the reference): the same mesh with shared vertices;
        // -smooth=N (N > 0): that mesh after N Taubin iterations; -decimate=C (C > 0): the welded
        // (and smoothed) mesh reduced by vertex clustering; -refine=B: marching cubes with one vertex
        // per cut edge, moved to where the edge leaves the masks' visual hull
        // -relax=N: the mesh one of those would write (welded where none is named), relaxed on the device
        const bool relax = !parser.str("relax").empty();
        const int base_source = !parser.str("refine").empty() ? ARVX_MESH_REFINED
                                : parser.i("decimate") > 0    ? ARVX_MESH_DECIMATED
                                : parser.i("smooth") > 0      ? ARVX_MESH_SMOOTHED
                                                              : ARVX_MESH_WELDED;
        if (relax)
            arvx::detail::marching_cubes_write(
                &model, parser.f("scale"), modelTranslation, 0.5f, parser.str("outFile"), [&](arvx::Model *m, float t) {
                    if (base_source == ARVX_MESH_REFINED)
                        (void)arvx::marchingCubesMeshRefined(in.intr, m, in.views, parser.i("refine"), t);
                    else if (base_source == ARVX_MESH_DECIMATED)
                        (void)arvx::marchingCubesMeshDecimated(m, t, parser.i("decimate"), std::max(parser.i("smooth"), 0));
                    else if (base_source == ARVX_MESH_SMOOTHED)
                        (void)arvx::marchingCubesMeshSmoothed(m, t, parser.i("smooth"));
                    else
                        (void)arvx::marchingCubesMeshWelded(m, t);
                    return arvx::relaxMesh(m, base_source, parser.i("relax"));
                });
        else if (!parser.str("refine").empty())
            arvx::marchingCubesRefined(in.intr, &model, in.views, parser.i("refine"), parser.f("scale"),
                                       modelTranslation, 0.5f, parser.str("outFile"));
        else if (parser.i("decimate") > 0)
            arvx::marchingCubesDecimated(&model, parser.f("scale"), modelTranslation, 0.5f, parser.str("outFile"),
                                         parser.i("decimate"), std::max(parser.i("smooth"), 0));
        else if (parser.i("smooth") > 0)
            arvx::marchingCubesSmoothed(&model, parser.f("scale"), modelTranslation, 0.5f,
                                        parser.str("outFile"), parser.i("smooth"));
        else if (parser.b("weld"))
            arvx::marchingCubesWelded(&model, parser.f("scale"), modelTranslation, 0.5f,
                                      parser.str("outFile"));
        else
            arvx::marchingCubes(&model, parser.f("scale"), modelTranslation, 0.5f, parser.str("outFile"));
        // -render=DIR (an extension beyond the reference): the welded mesh's vertex voxels drawn
        // into every view over its input image, then each render's agreement with the view's mask
        // -renderMesh=true: the triangles of the mesh written above instead, with a headlight
        const int mesh_source = !parser.b("renderMesh")          ? -1
                                : relax                          ? ARVX_MESH_RELAXED
                                : !parser.str("refine").empty() ? ARVX_MESH_REFINED
                                : parser.i("decimate") > 0      ? ARVX_MESH_DECIMATED
                                : parser.i("smooth") > 0        ? ARVX_MESH_SMOOTHED
                                                                : ARVX_MESH_WELDED;
        // -meshColor=closest|average: that mesh's vertices coloured from the images first, and drawn so
        int drawn = mesh_source;
        const std::string meshColor = parser.str("meshColor");
        if (!meshColor.empty()) {
            if (meshColor != "closest" && meshColor != "average") {
                std::cerr << "-meshColor takes closest or average" << std::endl;
                return 1;
            }
            if (mesh_source < 0 || parser.str("render").empty()) {
                std::cerr << "-meshColor needs -render=DIR and -renderMesh=true" << std::endl;
                return 1;
            }
            const arvx::MeshColors col = arvx::colorMesh(
                in.intr, &model, in.views, mesh_source, meshColor == "closest" ? ARVX_COLOR_CLOSEST : ARVX_COLOR_AVERAGE,
                tol * model.getSize(), parser.b("meshForeground") ? ARVX_MESH_COLOR_FOREGROUND : 0u);
            std::cout << "LOG - MESH COLOR: " << col.coloured << " of " << col.views.size()
                      << " vertices coloured from the images" << std::endl;
            drawn = mesh_source | ARVX_MESH_IMAGE_COLORS;
        }
        // -texture=R -atlasWidth=AW: the mesh written above textured from the images, written beside the
        // OFF file with the OFF file's own vertices, and drawn by the renders
        if (parser.i("texture") != 0) {
            const int source = relax                         ? ARVX_MESH_RELAXED
                               : !parser.str("refine").empty() ? ARVX_MESH_REFINED
                               : parser.i("decimate") > 0    ? ARVX_MESH_DECIMATED
                               : parser.i("smooth") > 0      ? ARVX_MESH_SMOOTHED
                               : parser.b("weld")            ? ARVX_MESH_WELDED
                                                             : -1;
            if (source < 0) {
                std::cerr << "-texture needs a mesh with shared vertices: -weld, -smooth, -decimate, -refine or -relax" << std::endl;
                return 1;
            }
            if (!meshColor.empty()) {
                std::cerr << "-texture and -meshColor exclude each other" << std::endl;
                return 1;
            }
            const arvx::MeshTexture tex = arvx::textureMesh(
                in.intr, &model, in.views, source, parser.i("texture"), parser.i("atlasWidth"), tol * model.getSize(),
                parser.b("meshForeground") ? ARVX_MESH_TEXTURE_FOREGROUND : 0u);
            std::cout << "LOG - MESH TEXTURE: " << tex.textured << " of " << tex.faces << " faces textured from the images, atlas "
                      << tex.width << " x " << tex.height << std::endl;
            std::vector<float> verts;
            std::vector<unsigned> faces;
            const fs::path off(parser.str("outFile"));
            if (!read_off(off.string(), verts, faces) || faces.size() != 3 * (size_t)tex.faces ||
                !arvx::writeOBJ(fs::path(off).replace_extension(".obj").string(), verts.data(), verts.size() / 3, faces.data(),
                                faces.size() / 3, 3, tex)) {
                std::cerr << "Could not write the textured mesh beside " << off.string() << " (--texture)" << std::endl;
                return 1;
            }
            if (mesh_source >= 0) drawn = mesh_source | ARVX_MESH_TEXTURED;
        }
        // -near=D: the triangle renders' near plane (the library refuses an invalid one)
        if (mesh_source >= 0 && !parser.str("render").empty() && parser.str("near") != "0")
            arvx::setRenderNear(&model, parser.f("near"));
        if (!parser.str("render").empty() && !render_views(parser.str("render"), in, model, drawn)) return 1;
    } catch (const arvx::Error &e) {
        return 3;  // (already logged)
    }
    return 0;
}
