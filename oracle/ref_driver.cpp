// ref_driver.cpp -- runs the reference program's own functions on a scene file.
//
// TEST INFRASTRUCTURE ONLY.  Compiled by oracle/Makefile together with the reference's
// Model.cpp, VoxelCarving.cpp, ColorReconstruction.cpp, Postprocessing3d.cpp and
// MarchingCubes.cpp (read in place from the reference checkout, never copied) against the
// stand-in headers of oracle/ref_standins/ into oracle/_ref/arvx_ref.  No GPU, no libarvx.
//
// Usage: arvx_ref SCENE
//
// SCENE is a text header, one statement per line, closed by a line `end`; after it come the raw
// pixels, per view a 3-channel mask (H*W*3 bytes) and then a BGR image (H*W*3 bytes):
//
//   dims X Y Z              grid extents
//   voxel S                 voxel size (float)
//   image W H               size of every mask and image
//   K k00 k01 ... k22       camera matrix, nine doubles, row major
//   view rx ry rz tx ty tz  one per view: rvec and tvec (doubles), what the marker board would
//                           have given for that view's image
//   assoc 0|1               grouping of the M * world row sums (arvx_ref_cv.hpp, G2); default 1
//   log FILE                where the reference's stdout chatter goes (default: dropped)
//   poses FILE              write, per view, intr (9 f32) and pose (12 f32), obtained as the
//                           reference obtains them
//   op ...                  the ops, run in order on ONE Model(X, Y, Z, S):
//      carve | fastCarve | closest | avg | handleUnseen | closure K
//      mc SCALE DX DY DZ THRESH FILE
//      load_model FILE      N x 4 f32 (RGBA) then N bytes (seen), N = X*Y*Z in the order of
//                           x + X*(y + Y*z); applied through Model::set and Model::visit
//      dump FILE            same layout, read through Model::get and Model::visited
//   end
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ColorReconstruction.h"
#include "MarchingCubes.h"
#include "Model.h"
#include "aruco_samples_utility.hpp"  // before PoseEstimation.h, which needs its names
#include "PoseEstimation.h"
#include "Postprocessing3d.h"
#include "VoxelCarving.h"

namespace {

std::streambuf* g_terminal = nullptr;  // std::cout's own buffer while the log has its place

void restore_cout() {
    if (g_terminal) std::cout.rdbuf(g_terminal);
    g_terminal = nullptr;
}

[[noreturn]] void die(const std::string& what) {
    restore_cout();
    std::cerr << "arvx_ref: " << what << std::endl;
    std::exit(1);
}

struct Op {
    std::string name;
    std::vector<std::string> args;
};

void load_model(Model& model, const std::string& file) {
    const int X = model.getX(), Y = model.getY(), Z = model.getZ();
    const size_t N = (size_t)X * Y * Z;
    std::vector<float> rgba(N * 4);
    std::vector<uint8_t> seen(N);
    std::ifstream in(file, std::ios::binary);
    if (!in) die("cannot open " + file);
    in.read(reinterpret_cast<char*>(rgba.data()), (std::streamsize)(N * 16));
    in.read(reinterpret_cast<char*>(seen.data()), (std::streamsize)N);
    if (!in) die("short model file " + file);
    for (int z = 0; z < Z; ++z)
        for (int y = 0; y < Y; ++y)
            for (int x = 0; x < X; ++x) {
                const size_t i = (size_t)x + (size_t)X * ((size_t)y + (size_t)Y * z);
                model.set(x, y, z, Vector4f(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]));
                if (seen[i]) model.visit(cv::Vec3i(x, y, z));
            }
}

void dump_model(Model& model, const std::string& file) {
    const int X = model.getX(), Y = model.getY(), Z = model.getZ();
    const size_t N = (size_t)X * Y * Z;
    std::vector<float> rgba(N * 4);
    std::vector<uint8_t> seen(N);
    for (int z = 0; z < Z; ++z)
        for (int y = 0; y < Y; ++y)
            for (int x = 0; x < X; ++x) {
                const size_t i = (size_t)x + (size_t)X * ((size_t)y + (size_t)Y * z);
                const Vector4f v = model.get(x, y, z);
                for (int k = 0; k < 4; ++k) rgba[4 * i + k] = v(k);
                seen[i] = model.visited(cv::Vec3i(x, y, z)) ? 1 : 0;
            }
    std::ofstream out(file, std::ios::binary);
    if (!out) die("cannot write " + file);
    out.write(reinterpret_cast<const char*>(rgba.data()), (std::streamsize)(N * 16));
    out.write(reinterpret_cast<const char*>(seen.data()), (std::streamsize)N);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) die("usage: arvx_ref SCENE");
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) die(std::string("cannot open ") + argv[1]);

    int X = 0, Y = 0, Z = 0, W = 0, H = 0;
    float voxel = 1.f;
    double K[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::vector<cv::Vec3d> rvecs, tvecs;
    std::vector<Op> ops;
    std::string log_file, pose_file, line;
    bool closed = false;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string key;
        if (!(ss >> key)) continue;
        if (key == "end") {
            closed = true;
            break;
        } else if (key == "dims") {
            ss >> X >> Y >> Z;
        } else if (key == "voxel") {
            std::string t;
            ss >> t;
            voxel = std::strtof(t.c_str(), nullptr);
        } else if (key == "image") {
            ss >> W >> H;
        } else if (key == "K") {
            for (int i = 0; i < 9; ++i) {
                std::string t;
                ss >> t;
                K[i] = std::strtod(t.c_str(), nullptr);
            }
        } else if (key == "view") {
            double v[6] = {0, 0, 0, 0, 0, 0};
            for (int i = 0; i < 6; ++i) {
                std::string t;
                ss >> t;
                v[i] = std::strtod(t.c_str(), nullptr);
            }
            rvecs.push_back(cv::Vec3d(v[0], v[1], v[2]));
            tvecs.push_back(cv::Vec3d(v[3], v[4], v[5]));
        } else if (key == "assoc") {
            int a = 1;
            ss >> a;
            cv::arvx_ref::assoc_left() = a ? 1 : 0;
        } else if (key == "log") {
            ss >> log_file;
        } else if (key == "poses") {
            ss >> pose_file;
        } else if (key == "op") {
            Op op;
            ss >> op.name;
            std::string a;
            while (ss >> a) op.args.push_back(a);
            ops.push_back(op);
        } else {
            die("unknown statement: " + key);
        }
        if (ss.fail() && !ss.eof()) die("malformed statement: " + line);
    }
    if (!closed) die("scene header has no `end`");
    if (X <= 0 || Y <= 0 || Z <= 0) die("dims missing");

    // the reference's chatter goes to the log, not the terminal
    std::ofstream log_stream;
    if (!log_file.empty()) log_stream.open(log_file);
    std::ostringstream dropped;
    std::streambuf* sink = dropped.rdbuf();
    if (log_stream.is_open()) sink = log_stream.rdbuf();
    g_terminal = std::cout.rdbuf(sink);

    const int V = (int)rvecs.size();
    std::vector<cv::Mat> images, masks;
    for (int v = 0; v < V; ++v) {
        if (W <= 0 || H <= 0) die("views need `image W H`");
        cv::Mat mask(H, W, CV_8UC3), image(H, W, CV_8UC3);
        in.read(reinterpret_cast<char*>(mask.data), (std::streamsize)H * W * 3);
        in.read(reinterpret_cast<char*>(image.data), (std::streamsize)H * W * 3);
        if (!in) die("scene holds fewer pixels than its views need");
        cv::arvx_ref::register_pose(image, rvecs[v], tvecs[v]);
        masks.push_back(mask);
        images.push_back(image);
    }

    cv::Mat cameraMatrix(3, 3, CV_64F);
    for (int i = 0; i < 9; ++i) cameraMatrix.at<double>(i / 3, i % 3) = K[i];
    cv::Mat distCoeffs(1, 5, CV_64F);  // all zero: cv::undistort is an exact copy

    if (!pose_file.empty()) {
        // intr and pose exactly as carve / fastCarve / voxel_pass obtain them
        cv::Mat intr = cameraMatrix.clone();
        intr.convertTo(intr, CV_32F);
        std::ofstream out(pose_file, std::ios::binary);
        if (!out) die("cannot write " + pose_file);
        for (int v = 0; v < V; ++v) {
            cv::Mat pose = estimatePoseFromImage(cameraMatrix, distCoeffs, images[v], false).inv()(cv::Rect(0, 0, 4, 3));
            float buf[21];
            for (int i = 0; i < 9; ++i) buf[i] = intr.at<float>(i / 3, i % 3);
            for (int i = 0; i < 12; ++i) buf[9 + i] = pose.at<float>(i / 4, i % 4);
            out.write(reinterpret_cast<const char*>(buf), sizeof buf);
        }
    }

    Model model(X, Y, Z, voxel);
    for (const Op& op : ops) {
        const std::vector<std::string>& a = op.args;
        if (op.name == "carve") {
            carve(cameraMatrix, distCoeffs, model, images, masks);
        } else if (op.name == "fastCarve") {
            fastCarve(cameraMatrix, distCoeffs, model, images, masks);
        } else if (op.name == "closest") {
            reconstructClosestColor(cameraMatrix, distCoeffs, model, images, masks);
        } else if (op.name == "avg") {
            reconstructAvgColor(cameraMatrix, distCoeffs, model, images, masks);
        } else if (op.name == "handleUnseen") {
            model.handleUnseen();
        } else if (op.name == "closure" && a.size() == 1) {
            if (applyClosure(&model, std::atoi(a[0].c_str())) != 0) die("applyClosure refused " + a[0]);
        } else if (op.name == "mc" && a.size() == 6) {
            const float scale = std::strtof(a[0].c_str(), nullptr);
            const Vector3f tr(std::strtof(a[1].c_str(), nullptr), std::strtof(a[2].c_str(), nullptr),
                              std::strtof(a[3].c_str(), nullptr));
            if (!marchingCubes(&model, scale, tr, std::strtof(a[4].c_str(), nullptr), a[5]))
                die("marchingCubes could not write " + a[5]);
        } else if (op.name == "load_model" && a.size() == 1) {
            load_model(model, a[0]);
        } else if (op.name == "dump" && a.size() == 1) {
            dump_model(model, a[0]);
        } else {
            die("unknown or malformed op: " + op.name);
        }
    }
    std::cout.flush();
    restore_cout();
    return 0;
}
