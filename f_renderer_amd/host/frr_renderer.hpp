// frr_renderer.hpp -- header-only C++17 host mirror of the reference's rasterization interface
// over the C ABI of include/frr.h (libfrr_hip.so).  No Rust toolchain exists in this image, so this
// is the compiled-language host layer: same names, argument meaning and error behaviour as
//   Renderer::geometry_processing  /root/reference/f_renderer/src/renderer.rs:96-112
//   Renderer::rasterization        /root/reference/f_renderer/src/renderer.rs:269-284
//   FrameBuffer::{new,fill,clear,get_size,get_data,set_pixel,get_pixel,draw_line}  renderer.rs:418-514, 540-588
//   set_identity / set_look_at / set_perspective   matrix_util.rs:3-35,   Camera  camera.rs:4-26
//   Model::{new,faces_len,vert,uv,normal}  obj_loader.rs:7-97 (+ init_vertex_input, phong.rs:187-201)
//   FrameBuffer::load_file  renderer.rs:427-471 (BGRA storage; TGA decoded here, the reference uses the image crate)
// batched at the granularity of the reference's draw loop (examples/src/bin/phong.rs:314-387) and
// with table-selected shaders instead of closures.  What panics in the reference throws frr::Error.
// All arithmetic of the path runs on the GPU inside libfrr_hip.so; this file is plumbing.
#pragma once
#include <array>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/frr.h"

namespace frr {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error("frr error " + std::to_string(c) + ": " + m), code(c) {}
};

using Mat4 = std::array<float, 16>; // column-major, as glam::Mat4::from_cols_array
struct Vec3 { float x, y, z; };

inline Mat4 set_identity() { Mat4 m; frr_set_identity(m.data()); return m; }                       // matrix_util.rs:3-8
inline Mat4 set_look_at(Vec3 eye, Vec3 at, Vec3 up)                                                // matrix_util.rs:10-22
{
    Mat4 m; const float e[3] = {eye.x, eye.y, eye.z}, a[3] = {at.x, at.y, at.z}, u[3] = {up.x, up.y, up.z};
    frr_set_look_at(e, a, u, m.data());
    return m;
}
inline Mat4 set_perspective(float fovy, float aspect, float zn, float zf)                          // matrix_util.rs:24-35
{
    Mat4 m; frr_set_perspective(fovy, aspect, zn, zf, m.data()); return m;
}

struct Camera {                                                                                    // camera.rs:4-26
    Vec3 eye, at, up;
    Mat4 mat_look_at;
    Camera(Vec3 e, Vec3 a, Vec3 u) : eye(e), at(a), up(u), mat_look_at(set_look_at(e, a, u)) {}
    const Mat4 &cal_look_at() { mat_look_at = set_look_at(eye, at, up); return mat_look_at; }
};

// Host image with the reference's FrameBuffer surface: RGBA8 row-major, offset (y*width + x)*4.
class FrameBuffer {
public:
    FrameBuffer(uint32_t width, uint32_t height) : width_(width), height_(height), buffer_((size_t)width * height * 4, 0) {}
    static FrameBuffer create(uint32_t width, uint32_t height) { return FrameBuffer(width, height); } // FrameBuffer::new
    // FrameBuffer::load_file (renderer.rs:427-471): decoded image rows top-down, Rgb8 / Rgba8 only, stored B,G,R,A
    // (alpha 255 for Rgb8); anything else panics in the reference -> frr::Error.  `pixels`: h x w x channels bytes.
    static FrameBuffer from_image(const uint8_t *pixels, uint32_t width, uint32_t height, int channels)
    {
        if (channels != 3 && channels != 4) throw Error(FRR_ERR_INVALID, "invalid color type (renderer.rs:461-463)");
        FrameBuffer fb(width, height);
        for (size_t i = 0; i < (size_t)width * height; ++i) {
            const uint8_t *c = pixels + i * channels;
            uint8_t *o = &fb.buffer_[i * 4];
            o[0] = c[2]; o[1] = c[1]; o[2] = c[0]; o[3] = channels == 4 ? c[3] : 255;             // :442-445, :454-457
        }
        return fb;
    }
    // True-colour TGA (types 2 and 10 = RLE, 24 or 32 bpp; the reference's assets are .tga, phong.rs:167-171)
    static FrameBuffer load_file(const std::string &path)
    {
        std::ifstream f(path, std::ios::binary);
        if (!f) throw Error(FRR_ERR_INVALID, "cannot open " + path + " (image::open(..).unwrap() panics)");
        const std::vector<uint8_t> d((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (d.size() < 18) throw Error(FRR_ERR_INVALID, "truncated TGA header");
        const int idlen = d[0], cmap = d[1], typ = d[2], bpp = d[16], desc = d[17];
        const uint32_t w = d[12] | (d[13] << 8), h = d[14] | (d[15] << 8);
        if (cmap != 0 || (typ != 2 && typ != 10) || (bpp != 24 && bpp != 32)) throw Error(FRR_ERR_UNSUPPORTED, "unsupported TGA (true-colour 24/32 bpp, types 2 and 10 only)");
        const size_t n = (size_t)w * h, bp = bpp / 8;
        size_t pos = 18 + idlen;
        std::vector<uint8_t> raw(n * bp);
        auto need = [&](size_t k) { if (pos + k > d.size()) throw Error(FRR_ERR_INVALID, "truncated TGA data"); };
        if (typ == 2) {
            need(n * bp);
            std::memcpy(raw.data(), &d[pos], n * bp);
        } else {
            for (size_t i = 0; i < n;) {
                need(1);
                const int hdr = d[pos++];
                const size_t cnt = (size_t)(hdr & 0x7F) + 1;
                if (i + cnt > n) throw Error(FRR_ERR_INVALID, "TGA run leaves the image");
                if (hdr & 0x80) {
                    need(bp);
                    for (size_t k = 0; k < cnt; ++k) std::memcpy(&raw[(i + k) * bp], &d[pos], bp);
                    pos += bp;
                } else {
                    need(cnt * bp);
                    std::memcpy(&raw[i * bp], &d[pos], cnt * bp);
                    pos += cnt * bp;
                }
                i += cnt;
            }
        }
        // file order is B,G,R(,A), rows bottom-up unless descriptor bit 5, columns right-to-left if bit 4
        std::vector<uint8_t> img(n * bp);
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const uint32_t sy = (desc & 0x20) ? y : h - 1 - y, sx = (desc & 0x10) ? w - 1 - x : x;
                const uint8_t *s = &raw[((size_t)sy * w + sx) * bp];
                uint8_t *o = &img[((size_t)y * w + x) * bp];
                o[0] = s[2]; o[1] = s[1]; o[2] = s[0];
                if (bp == 4) o[3] = s[3];
            }
        return from_image(img.data(), w, h, (int)bp);
    }
    uint32_t width() const { return width_; }
    uint32_t height() const { return height_; }
    const std::vector<uint8_t> &get_data() const { return buffer_; }
    std::vector<uint8_t> &get_data_mut() { return buffer_; }
    uint32_t get_size() const { return width_ * height_ * 4; }
    void clear() { std::fill(buffer_.begin(), buffer_.end(), 0); }
    void fill(const std::array<uint8_t, 4> &c) { for (size_t i = 0; i < buffer_.size(); i += 4) std::memcpy(&buffer_[i], c.data(), 4); }
    void set_pixel(uint32_t x, uint32_t y, const std::array<uint8_t, 4> &c) { std::memcpy(&buffer_.at((size_t)(y * width_ + x) * 4 + 0), c.data(), 4); }
    std::array<uint8_t, 4> get_pixel(uint32_t x, uint32_t y) const
    {
        std::array<uint8_t, 4> c;
        std::memcpy(c.data(), &buffer_.at((size_t)(y * width_ + x) * 4), 4);
        return c;
    }
    // renderer.rs:540-588, statement by statement: endpoints sorted per axis, independently (a falling line is drawn as the
    // rising one); vertical / horizontal lines exclude their upper end; set_pixel addresses linearly with no test of x, so
    // x >= width lands in a later row, and past the buffer the reference panics (std::out_of_range here)
    void draw_line(uint32_t xa, uint32_t ya, uint32_t xb, uint32_t yb, const std::array<uint8_t, 4> &c)
    {
        const uint32_t x1 = xa < xb ? xa : xb, x2 = xa < xb ? xb : xa, y1 = ya < yb ? ya : yb, y2 = ya < yb ? yb : ya;
        auto put = [&](uint64_t x, uint64_t y) {
            const uint64_t p = y * width_ + x;
            if (p >= (uint64_t)width_ * height_) throw std::out_of_range("draw_line: pixel past the buffer");
            std::memcpy(&buffer_[(size_t)p * 4], c.data(), 4);
        };
        if (x1 == x2 && y1 == y2) put(x1, y1);
        else if (x1 == x2) for (uint64_t y = y1; y < y2; ++y) put(x1, y);
        else if (y1 == y2) for (uint64_t x = x1; x < x2; ++x) put(x, y1);
        else {
            const uint64_t dx = x2 - x1, dy = y2 - y1;
            uint64_t rem = 0;
            if (dx > dy) {
                uint64_t y = y1;
                for (uint64_t x = x1; x < x2; ++x) { put(x, y); rem += dy; if (rem >= dx) { y += 1; rem -= dx; put(x, y); } }
            } else {
                uint64_t x = x1;
                for (uint64_t y = y1; y < y2; ++y) { put(x, y); rem += dx; if (rem >= dy) { x += 1; rem -= dy; put(x, y); } }
            }
            put(x2, y2);
        }
    }
private:
    uint32_t width_, height_;
    std::vector<uint8_t> buffer_;
};

struct VSInput { float pos[3]; float uv[2]; float normal[3]; };          // phong.rs:49-54 (FRR_VS_PHONG / GOURAUD)
static_assert(sizeof(VSInput) == 32, "VSInput must be 8 packed floats");

// obj_loader.rs:7-97.  Lines are split on "\n", tokens on SINGLE spaces (consecutive spaces give empty tokens, as
// in the reference), "\r" is stripped from the tokens that are parsed; only v / vn / vt / f lines are used; a face
// takes its first three a/b/c triples (1-based -> 0-based); normals are normalised when fetched (:93-96).  Every
// `.unwrap()` / index panic of the reference is an frr::Error here.  (Invalid UTF-8 is replaced in the reference,
// :28; such bytes can only sit in lines or tokens that are never parsed as numbers, so they need no handling.)
class Model {
public:
    explicit Model(const std::string &path)
    {
        std::ifstream f(path, std::ios::binary);
        if (!f) throw Error(FRR_ERR_INVALID, "cannot open " + path + " (File::open(..).unwrap() panics, obj_loader.rs:24)");
        const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        parse(text);
    }
    static Model from_text(const std::string &text) { Model m; m.parse(text); return m; }
    size_t faces_len() const { return faces_.size(); }                                                     // :79-81
    Vec3 vert(size_t i_face, size_t nth) const { return at(verts_, faces_.at(i_face)[nth][0]); }           // :83-86
    std::array<float, 2> uv(size_t i_face, size_t nth) const { return at(uv_, faces_.at(i_face)[nth][1]); } // :88-91
    Vec3 normal(size_t i_face, size_t nth) const                                                           // :93-96
    {
        const Vec3 n = at(norms_, faces_.at(i_face)[nth][2]);
        const float dot = (n.x * n.x + n.y * n.y) + n.z * n.z;        // glam Vec3::normalize = self * (1 / sqrt(dot))
        const float r = 1.0f / std::sqrt(dot);
        return Vec3{n.x * r, n.y * r, n.z * r};
    }
    // init_vertex_input (phong.rs:187-201): Vec<[VSInput;3]>
    std::vector<std::array<struct VSInput, 3>> vertex_inputs() const;
    // The same mesh without the expansion, for Renderer::upload_mesh_indexed: one VSInput per distinct (v, vt, vn) triple of
    // the faces, in first-use order, and per face the three vertex numbers.  vertices[faces[i][j]] == vertex_inputs()[i][j],
    // bit for bit.
    struct Indexed { std::vector<struct VSInput> vertices; std::vector<std::array<uint32_t, 3>> faces; };
    Indexed indexed_inputs() const;

private:
    Model() = default;
    template <class T> static const T &at(const std::vector<T> &v, uint32_t i)
    {
        if (i >= v.size()) throw Error(FRR_ERR_INVALID, "OBJ index out of bounds (the reference panics)");
        return v[i];
    }
    static std::vector<std::string> split(const std::string &s, char sep)
    {
        std::vector<std::string> out;
        size_t b = 0;
        for (;;) {
            const size_t e = s.find(sep, b);
            out.push_back(s.substr(b, e == std::string::npos ? std::string::npos : e - b));
            if (e == std::string::npos) break;
            b = e + 1;
        }
        return out;
    }
    static std::string strip_cr(std::string t) { std::string o; for (char c : t) if (c != '\r') o.push_back(c); return o; }
    static const std::string &tok(const std::vector<std::string> &l, size_t i)
    {
        if (i >= l.size()) throw Error(FRR_ERR_INVALID, "OBJ line has too few tokens (index panic in the reference)");
        return l[i];
    }
    static float parse_f32(const std::string &raw)     // str::parse::<f32>() after .replace("\r", "")
    {
        const std::string t = strip_cr(raw);
        bool ok = !t.empty();
        for (char c : t) ok = ok && (std::isdigit((unsigned char)c) || c == '.' || c == '-' || c == '+' || c == 'e' || c == 'E' ||
                                     std::isalpha((unsigned char)c)); // letters: inf / nan / infinity spellings, checked below
        char *end = nullptr;
        const float v = ok ? std::strtof(t.c_str(), &end) : 0.0f;
        if (!ok || end != t.c_str() + t.size() || t.find_first_of("xXpP") != std::string::npos)
            throw Error(FRR_ERR_INVALID, "invalid f32 literal '" + t + "' (parse::<f32>().unwrap() panics)");
        return v;
    }
    static uint32_t parse_u32_minus_1(const std::string &raw)  // parse::<u32>().unwrap() - 1 (:62-64)
    {
        const std::string t = strip_cr(raw);
        size_t b = (!t.empty() && t[0] == '+') ? 1 : 0;
        bool ok = t.size() > b;
        unsigned long long v = 0;
        for (size_t i = b; i < t.size() && ok; ++i) { ok = std::isdigit((unsigned char)t[i]) != 0; v = v * 10 + (unsigned)(t[i] - '0'); if (v > 0xFFFFFFFFull) ok = false; }
        if (!ok || v == 0) throw Error(FRR_ERR_INVALID, "invalid u32 index '" + t + "' (parse / `- 1` underflow panics in the reference)");
        return (uint32_t)(v - 1);
    }
    void parse(const std::string &text)
    {
        for (const std::string &line : split(text, '\n')) {                                                // :29
            const std::vector<std::string> l = split(line, ' ');                                           // :32
            const std::string &tag = l[0];
            if (tag == "v") verts_.push_back(Vec3{parse_f32(tok(l, 1)), parse_f32(tok(l, 2)), parse_f32(tok(l, 3))});       // :37-43
            else if (tag == "vn") norms_.push_back(Vec3{parse_f32(tok(l, 1)), parse_f32(tok(l, 2)), parse_f32(tok(l, 3))}); // :44-50
            else if (tag == "vt") uv_.push_back({parse_f32(tok(l, 1)), parse_f32(tok(l, 2))});                              // :51-56
            else if (tag == "f") {                                                                                          // :57-69
                std::array<std::array<uint32_t, 3>, 3> tri;
                for (int i = 1; i < 4; ++i) {
                    const std::vector<std::string> vv = split(tok(l, i), '/');
                    tri[i - 1] = {parse_u32_minus_1(tok(vv, 0)), parse_u32_minus_1(tok(vv, 1)), parse_u32_minus_1(tok(vv, 2))};
                }
                faces_.push_back(tri);
            }
        }
    }
    std::vector<Vec3> verts_, norms_;
    std::vector<std::array<float, 2>> uv_;
    std::vector<std::array<std::array<uint32_t, 3>, 3>> faces_;
};

inline std::vector<std::array<VSInput, 3>> Model::vertex_inputs() const
{
    std::vector<std::array<VSInput, 3>> out(faces_len());
    for (size_t i = 0; i < faces_len(); ++i)
        for (size_t j = 0; j < 3; ++j) {
            const Vec3 p = vert(i, j), n = normal(i, j);
            const std::array<float, 2> t = uv(i, j);
            out[i][j] = VSInput{{p.x, p.y, p.z}, {t[0], t[1]}, {n.x, n.y, n.z}};
        }
    return out;
}

inline Model::Indexed Model::indexed_inputs() const
{
    Indexed out;
    out.faces.resize(faces_len());
    std::map<std::array<uint32_t, 3>, uint32_t> seen;
    for (size_t i = 0; i < faces_len(); ++i)
        for (size_t j = 0; j < 3; ++j) {
            const auto it = seen.find(faces_[i][j]);
            if (it != seen.end()) { out.faces[i][j] = it->second; continue; }
            const Vec3 p = vert(i, j), n = normal(i, j);
            const std::array<float, 2> t = uv(i, j);
            out.faces[i][j] = seen[faces_[i][j]] = (uint32_t)out.vertices.size();
            out.vertices.push_back(VSInput{{p.x, p.y, p.z}, {t[0], t[1]}, {n.x, n.y, n.z}});
        }
    return out;
}

struct Mesh { int id = -1; uint64_t ntris = 0; int vs = 0; };
struct Lines { int id = -1; uint64_t nlines = 0; };   // a list of draw_line calls on the device
struct Instances { int id = -1; uint64_t ninst = 0; };   // a table of model matrices on the device: one per instance of an instanced pass
struct Materials { int id = -1; uint64_t n = 0; };        // a table of frr_material on the device: the pixel uniforms of each item of a pass (shade_items)
struct DrawList { int id = -1; uint64_t nitems = 0; };   // (mesh, model matrix) items on the device: one list pass draws them all
struct LineSegment { uint32_t x1, y1, x2, y2; };
static_assert(sizeof(LineSegment) == 16, "LineSegment must be 4 packed u32");

// Device-resident FrameBuffer + f32 depth buffer + u32 triangle-id buffer and the two halves of the
// reference's draw loop as batched calls (`Renderer {}` itself is stateless in the reference, :41).
class Renderer {
public:
    Renderer(uint32_t width, uint32_t height, int device = 0, void *hip_stream = nullptr) : width_(width), height_(height)
    {
        int rc = frr_create(device, width, height, hip_stream, &ctx_);
        if (rc != FRR_OK) throw Error(rc, "frr_create failed (no gfx950 device, bad size or out of memory); there is no CPU fallback");
        std::memset(&uniforms, 0, sizeof uniforms);
        frr_set_identity(uniforms.model); frr_set_identity(uniforms.view); frr_set_identity(uniforms.proj);
        uniforms.light_pos[0] = 1.2f; uniforms.light_pos[1] = 1.0f; uniforms.light_pos[2] = 2.0f;          // phong.rs:129
        uniforms.light_color[0] = uniforms.light_color[1] = uniforms.light_color[2] = 1.0f;               // phong.rs:128
        uniforms.ambient_strength = 0.1f; uniforms.specular_strength = 0.5f;                              // phong.rs:131-132
        uniforms.flat_color[0] = uniforms.flat_color[1] = uniforms.flat_color[2] = uniforms.flat_color[3] = 1.0f;
    }
    ~Renderer() { if (ctx_) frr_destroy(ctx_); }
    Renderer(const Renderer &) = delete;
    Renderer &operator=(const Renderer &) = delete;

    uint32_t width() const { return width_; }
    uint32_t height() const { return height_; }
    frr_uniforms uniforms; // VSUniform + PSUniform (phong.rs:26-47); call set_uniforms() after editing

    // Vec<[VSInput;3]> (phong.rs:187-205)
    Mesh upload_mesh(const std::vector<std::array<VSInput, 3>> &tris, int vs_id = FRR_VS_PHONG)
    {
        return upload_mesh_raw(reinterpret_cast<const float *>(tris.data()), tris.size(), vs_id);
    }
    Mesh upload_mesh_raw(const float *vs_inputs, uint64_t ntris, int vs_id)
    {
        Mesh m; m.ntris = ntris; m.vs = vs_id;
        check(frr_mesh_upload(ctx_, vs_inputs, ntris, vs_id, &m.id));
        return m;
    }
    // The Model itself (vertex array + index list) instead of its expansion: corner j of triangle t is
    // vertices[faces[t][j]].  An index >= the vertex count is the reference's out-of-bounds panic -> frr::Error.
    Mesh upload_mesh_indexed(const Model::Indexed &m, int vs_id = FRR_VS_PHONG)
    {
        return upload_mesh_indexed_raw(reinterpret_cast<const float *>(m.vertices.data()), m.vertices.size(),
                                       reinterpret_cast<const uint32_t *>(m.faces.data()), m.faces.size(), vs_id);
    }
    Mesh upload_mesh_indexed_raw(const float *vertices, uint64_t nverts, const uint32_t *indices, uint64_t ntris, int vs_id)
    {
        Mesh m; m.ntris = ntris; m.vs = vs_id;
        check(frr_mesh_upload_indexed(ctx_, vertices, nverts, indices, ntris, vs_id, &m.id));
        return m;
    }
    // the same for device memory the caller owns (16-byte aligned vertices); validated on the device inside the call.  After
    // an in-place rewrite of either buffer: frame_fence, rewrite, bind again (include/frr.h: frr_create)
    Mesh bind_mesh_device_indexed(const void *dev_vertices, uint64_t nverts, const void *dev_indices, uint64_t ntris, int vs_id)
    {
        Mesh m; m.ntris = ntris; m.vs = vs_id;
        check(frr_mesh_bind_device_indexed(ctx_, dev_vertices, nverts, dev_indices, ntris, vs_id, &m.id));
        return m;
    }
    // A list of FrameBuffer::draw_line calls (renderer.rs:540-588), in call order.  A segment whose walk would leave the
    // buffer (the reference's panic) -> frr::Error naming it, and no list.
    // The model matrices of the objects that share a mesh (phong.rs:319-331: vs_uniform.model per object), column-major like
    // uniforms.model; bind_instances_device: a table already in device memory (16-byte aligned; after an in-place rewrite:
    // frame_fence, rewrite, bind again).
    Instances upload_instances(const std::vector<Mat4> &models)
    {
        Instances t; t.ninst = models.size();
        check(frr_instances_upload(ctx_, models.empty() ? nullptr : models[0].data(), t.ninst, &t.id));
        return t;
    }
    Instances bind_instances_device(const void *dev_models, uint64_t ninst)
    {
        Instances t; t.ninst = ninst;
        check(frr_instances_bind_device(ctx_, dev_models, ninst, &t.id));
        return t;
    }
    void free_instances(Instances &t) { if (t.id >= 0) { check(frr_instances_free(ctx_, t.id)); t.id = -1; } }
    // The pixel uniforms that change from object to object (phong.rs:34-47: ps_uniform.place per object), one frr_material per
    // item of a pass: texture slot, ambient and specular strength, flat colour, u.user[0 .. FRR_MATERIAL_USER).
    Materials upload_materials(const std::vector<frr_material> &mats)
    {
        Materials t; t.n = mats.size();
        check(frr_materials_upload(ctx_, mats.empty() ? nullptr : mats.data(), t.n, &t.id));
        return t;
    }
    Materials bind_materials_device(const void *dev_mats, uint64_t n)   // 16-byte aligned; checked on the device inside the call (a host wait)
    {
        Materials t; t.n = n;
        check(frr_materials_bind_device(ctx_, dev_mats, n, &t.id));
        return t;
    }
    void free_materials(Materials &t) { if (t.id >= 0) { check(frr_materials_free(ctx_, t.id)); t.id = -1; } }
    // The objects of a frame that do not share a mesh (phong.rs:319-359: body, face, hair), each under its own model matrix
    // (column-major like uniforms.model).  A snapshot of the meshes: freeing one of them kills the list.
    DrawList upload_draw_list(const std::vector<Mesh> &meshes, const std::vector<Mat4> &models)
    {
        if (meshes.size() != models.size()) throw Error(FRR_ERR_INVALID, "one model matrix per mesh");
        std::vector<frr_draw_item> items(meshes.size());
        for (size_t i = 0; i < items.size(); ++i) {
            items[i].mesh = meshes[i].id; items[i].reserved = 0;
            std::memcpy(items[i].model, models[i].data(), sizeof items[i].model);
        }
        DrawList l; l.nitems = items.size();
        check(frr_drawlist_upload(ctx_, items.empty() ? nullptr : items.data(), l.nitems, &l.id));
        return l;
    }
    void free_draw_list(DrawList &l) { if (l.id >= 0) { check(frr_drawlist_free(ctx_, l.id)); l.id = -1; } }
    Lines upload_lines(const std::vector<LineSegment> &segments, const std::vector<std::array<uint8_t, 4>> &colors)
    {
        if (segments.size() != colors.size()) throw Error(FRR_ERR_INVALID, "one colour per segment");
        Lines l; l.nlines = segments.size();
        check(frr_lines_upload(ctx_, reinterpret_cast<const uint32_t *>(segments.data()), reinterpret_cast<const uint8_t *>(colors.data()), l.nlines, &l.id));
        return l;
    }
    // the same for device memory the caller owns (segments 16-byte aligned); validated on the device inside the call
    Lines bind_lines_device(const void *dev_xyxy, const void *dev_rgba, uint64_t nlines)
    {
        Lines l; l.nlines = nlines;
        check(frr_lines_bind_device(ctx_, dev_xyxy, dev_rgba, nlines, &l.id));
        return l;
    }
    void free_lines(Lines &l) { if (l.id >= 0) { check(frr_lines_free(ctx_, l.id)); l.id = -1; } }
    // frame_buffer.draw_line(...) for every segment of the list, in order: colour only, ordered with the draws around it
    void draw_lines(const Lines &l) { check(frr_draw_lines(ctx_, l.id)); }
    // the edges of every triangle of the last geometry_processing / draw in one colour (an edge with an endpoint off the
    // screen is skipped whole); no read-back
    void draw_wireframe(const std::array<uint8_t, 4> &color) { check(frr_draw_wireframe(ctx_, color.data())); }
    void free_mesh(Mesh &m) { if (m.id >= 0) { check(frr_mesh_free(ctx_, m.id)); m.id = -1; } }
    void set_texture(int slot, const FrameBuffer &fb) { check(frr_texture_upload(ctx_, slot, fb.get_data().data(), fb.width(), fb.height())); }
    void set_uniforms() { check(frr_set_uniforms(ctx_, &uniforms)); }
    // The reference's closure shaders (renderer.rs:105,283) as HIP text compiled at run time (include/frr.h: user shaders):
    // returns the id to upload a mesh with (vs_id) and to draw it with (pixel_shader).
    int register_shader(const std::string &hip_source, int vs_input_floats, int num_varyings)
    {
        int id = -1;
        check(frr_shader_register(ctx_, hip_source.c_str(), vs_input_floats, num_varyings, &id));
        return id;
    }
    void set_user_uniforms(const std::vector<float> &v) { check(frr_set_user_uniforms(ctx_, v.data(), (int)v.size())); }   // what the closures would capture
    void set_option(const char *name, int64_t value) { check(frr_set_option(ctx_, name, value)); }   // dev / test switches, include/frr.h
    void set_partition(int rank, int world, bool blocked = false)
    {
        check(frr_set_partition(ctx_, rank, world));
        check(frr_set_partition_layout(ctx_, blocked ? 1 : 0));
    }

    // frame_buffer.fill(color); depth_buffer.fill(depth)   (phong.rs:316-317)
    void clear(const std::array<uint8_t, 4> &color = {30, 30, 30, 255}, float depth = 0.0f) { check(frr_clear(ctx_, color.data(), depth)); }
    // loop A (phong.rs:321-331)
    void geometry_processing(const Mesh &m) { check(frr_geometry(ctx_, m.id, nullptr)); }
    // loop B (phong.rs:361-381); width_range / height_range as renderer.rs:270-271
    void rasterization(std::pair<int32_t, int32_t> width_range, std::pair<int32_t, int32_t> height_range, int pixel_shader)
    {
        check(frr_raster(ctx_, pixel_shader, width_range.first, width_range.second, height_range.first, height_range.second));
    }
    void draw(const Mesh &m, int pixel_shader)
    {
        check(frr_draw(ctx_, m.id, pixel_shader, 0, (int32_t)width_, 0, (int32_t)height_));
    }
    // Loop A under every matrix of the table in turn -- the loop over objects around it, phong.rs:319-331 -- into ONE setup list
    // in (instance, triangle) order; draw_instanced: that and one rasterization over the list.  Bit for bit what one
    // draw(mesh) per matrix gives with uniforms.model = that matrix.
    void geometry_processing_instanced(const Mesh &m, const Instances &t) { check(frr_geometry_instanced(ctx_, m.id, t.id, nullptr)); }
    void draw_instanced(const Mesh &m, const Instances &t, int pixel_shader)
    {
        check(frr_draw_instanced(ctx_, m.id, t.id, pixel_shader, 0, (int32_t)width_, 0, (int32_t)height_));
    }
    // Face culling of the geometry passes issued from now on (frr_set_cull): FRR_CULL_NONE, FRR_CULL_NEG (drop the inputs whose
    // clip-space determinant is < 0) or FRR_CULL_POS (> 0).  The reference has no such switch: the default draws everything.
    void set_cull(int mode) { check(frr_set_cull(ctx_, mode)); }
    // Loop A over every item's mesh under that item's matrix into ONE setup list in (item, triangle) order -- the whole setup
    // loop of phong.rs:319-359; draw_list: that and one rasterization over the list.  Bit for bit what one draw(mesh_i) per
    // item gives with uniforms.model = model_i.
    void geometry_list(const DrawList &l) { check(frr_geometry_list(ctx_, l.id, nullptr)); }
    void draw_list(const DrawList &l, int pixel_shader)
    {
        check(frr_draw_list(ctx_, l.id, pixel_shader, 0, (int32_t)width_, 0, (int32_t)height_));
    }
    // The same with every item i whose keep[i] < min_value (unsigned) replaced by an empty mesh (include/frr.h:
    // frr_geometry_list_if).  dev_keep_u32: device memory, one u32 per item -- what visible_pixels(FRR_PER_ITEM, dev, n) wrote
    // for the previous frame, or a 0/1 mask.  It is read on the library's streams behind every earlier command of this
    // renderer and behind pending frame_wait streams, with no host wait; keep it as it is until the next sync or clear.
    void geometry_list_if(const DrawList &l, const void *dev_keep_u32, uint64_t entries, uint32_t min_value = 1)
    {
        check(frr_geometry_list_if(ctx_, l.id, dev_keep_u32, entries, min_value, nullptr));
    }
    void draw_list_if(const DrawList &l, const void *dev_keep_u32, uint64_t entries, int pixel_shader, uint32_t min_value = 1)
    {
        check(frr_draw_list_if(ctx_, l.id, dev_keep_u32, entries, min_value, pixel_shader, 0, (int32_t)width_, 0, (int32_t)height_));
    }
    // per item of the latest geometry pass (list items, instances, or one for a plain pass): the triangle id of its first setup
    // triangle and how many it emitted -- body_offset / face_offset of phong.rs:333-359 without a read-back per draw
    void item_ranges(std::vector<uint32_t> &first, std::vector<uint32_t> &count)
    {
        uint64_t n = 0;
        check(frr_geometry_item_ranges(ctx_, nullptr, nullptr, 0, &n));
        first.assign((size_t)n, 0u); count.assign((size_t)n, 0u);
        if (n) check(frr_geometry_item_ranges(ctx_, first.data(), count.data(), n, &n));
    }
    static int64_t host_list_item(const std::vector<uint32_t> &first, const std::vector<uint32_t> &ntris, uint32_t t)
    {
        return first.size() == ntris.size() ? frr_host_list_item(first.data(), ntris.data(), first.size(), t) : -1;
    }
    // How many entries of the window each unit owns in the triangle-id target (include/frr.h: frr_visible_pixels): FRR_PER_ITEM,
    // the items of the latest geometry pass as item_ranges reports them, or FRR_PER_TRIANGLE, the triangle ids of the frame so
    // far -- which objects of a list ended up on screen, with no read-back of the frame.  Device memory of `entries` u32, every
    // one written; a command on the frame's stream, no host wait: order the reads with frame_fence on a created stream or with
    // sync, and keep the buffer until then.
    void visible_pixels(int unit, void *dev_out_u32, uint64_t entries, std::pair<int32_t, int32_t> width_range, std::pair<int32_t, int32_t> height_range)
    {
        check(frr_visible_pixels(ctx_, unit, width_range.first, width_range.second, height_range.first, height_range.second, dev_out_u32, entries));
    }
    void visible_pixels(int unit, void *dev_out_u32, uint64_t entries) { visible_pixels(unit, dev_out_u32, entries, {0, (int32_t)width_}, {0, (int32_t)height_}); }
    // the same on the host (a synchronisation point): the counts of all n units
    std::vector<uint32_t> visible_pixels(int unit, std::pair<int32_t, int32_t> width_range, std::pair<int32_t, int32_t> height_range)
    {
        return counts_on_host(frr_visible_pixels_host, unit, width_range, height_range);
    }
    std::vector<uint32_t> visible_pixels(int unit) { return visible_pixels(unit, {0, (int32_t)width_}, {0, (int32_t)height_}); }
    // The occlusion query (include/frr.h: frr_query_pixels): how many fragments of each unit of the latest geometry pass would
    // pass the depth test against the depth target as it stands -- nothing is drawn.  Device memory of `entries` u32, every one
    // written; a command on the frame's stream, no host wait.  The buffer is a keep buffer for draw_list_if as it is: that
    // pass is already ordered behind the query.
    void query_pixels(int unit, void *dev_out_u32, uint64_t entries, std::pair<int32_t, int32_t> width_range, std::pair<int32_t, int32_t> height_range)
    {
        check(frr_query_pixels(ctx_, unit, width_range.first, width_range.second, height_range.first, height_range.second, dev_out_u32, entries));
    }
    void query_pixels(int unit, void *dev_out_u32, uint64_t entries) { query_pixels(unit, dev_out_u32, entries, {0, (int32_t)width_}, {0, (int32_t)height_}); }
    // the same on the host (a synchronisation point): the counts of all n units
    std::vector<uint32_t> query_pixels(int unit, std::pair<int32_t, int32_t> width_range, std::pair<int32_t, int32_t> height_range)
    {
        return counts_on_host(frr_query_pixels_host, unit, width_range, height_range);
    }
    std::vector<uint32_t> query_pixels(int unit) { return query_pixels(unit, {0, (int32_t)width_}, {0, (int32_t)height_}); }
    // Box queries (include/frr.h: frr_drawlist_bounds, frr_query_boxes).  list_bounds: per item of the list the object-space box
    // of its mesh -- lo_hi: 6 floats per item, lo xyz then hi xyz -- and flags (bit 0: a non-finite position, bit 1: no
    // triangles), computed on the device; a synchronisation point.  The table stays with the list: query_boxes needs it.
    void list_bounds(const DrawList &list, std::vector<float> &lo_hi, std::vector<uint32_t> &flags)
    {
        uint64_t n = 0;
        lo_hi.assign((size_t)list.nitems * 6, 0.0f); flags.assign((size_t)list.nitems, 0u);
        check(frr_drawlist_bounds(ctx_, list.id, lo_hi.data(), flags.data(), list.nitems, &n));
    }
    void list_bounds(const DrawList &list) { check(frr_drawlist_bounds(ctx_, list.id, nullptr, nullptr, 0, nullptr)); }
    // query_boxes: per item 0 where its box lies behind the depth target as it stands or outside the window -- drawing the
    // item now would change nothing -- else an upper bound of the pixels it can own.  Conservative, not exact; no geometry
    // pass, no host wait.  The buffer is a keep buffer for draw_list_if as it is.
    void query_boxes(const DrawList &list, void *dev_out_u32, uint64_t entries, std::pair<int32_t, int32_t> width_range, std::pair<int32_t, int32_t> height_range)
    {
        check(frr_query_boxes(ctx_, list.id, width_range.first, width_range.second, height_range.first, height_range.second, dev_out_u32, entries));
    }
    void query_boxes(const DrawList &list, void *dev_out_u32, uint64_t entries) { query_boxes(list, dev_out_u32, entries, {0, (int32_t)width_}, {0, (int32_t)height_}); }
    // the same on the host (a synchronisation point): one value per item of the list
    std::vector<uint32_t> query_boxes(const DrawList &list, std::pair<int32_t, int32_t> width_range, std::pair<int32_t, int32_t> height_range)
    {
        std::vector<uint32_t> out((size_t)list.nitems, 0u);
        uint64_t n = 0;
        if (!out.empty()) check(frr_query_boxes_host(ctx_, list.id, width_range.first, width_range.second, height_range.first, height_range.second, out.data(), out.size(), &n));
        return out;
    }
    std::vector<uint32_t> query_boxes(const DrawList &list) { return query_boxes(list, {0, (int32_t)width_}, {0, (int32_t)height_}); }
    void sync() { check(frr_sync(ctx_)); }
    // stream-side ordering against a caller's hipStream_t (nullptr: the renderer's own), no host wait: frame_fence -- the stream
    // waits for every frame issued so far; frame_wait -- the next write of the frame targets waits for what the stream holds now
    void frame_fence(void *stream = nullptr) { check(frr_frame_fence(ctx_, stream)); }
    void frame_wait(void *stream = nullptr) { check(frr_frame_wait(ctx_, stream)); }

    // image_slice.copy_from_slice(frame_buffer.get_data())   (phong.rs:386)
    void read_frame_buffer(FrameBuffer &fb)
    {
        if (fb.width() != width_ || fb.height() != height_) throw Error(FRR_ERR_INVALID, "FrameBuffer size mismatch");
        check(frr_readback(ctx_, fb.get_data_mut().data(), nullptr, nullptr));
    }
    void read_depth(std::vector<float> &depth) { depth.resize((size_t)width_ * height_); check(frr_readback(ctx_, nullptr, depth.data(), nullptr)); }
    void read_triangle_ids(std::vector<uint32_t> &ids) { ids.resize((size_t)width_ * height_); check(frr_readback(ctx_, nullptr, nullptr, ids.data())); }
    // The pixel shader's input (renderer.rs:368-378) of every pixel of the window that a triangle of the last
    // geometry_processing / draw owns, f32 [entries][K] with entry (cy - y0) * x1 + (cx - x0); every other entry is left
    // untouched (include/frr.h: frr_resolve_varyings).  Device memory, no host wait: order the reads with frame_fence on a
    // created stream (nullptr / the legacy default stream means the renderer's own) or with sync.
    void resolve_varyings(void *dev_out_f32, uint64_t entries, std::pair<int32_t, int32_t> width_range, std::pair<int32_t, int32_t> height_range)
    {
        check(frr_resolve_varyings(ctx_, width_range.first, width_range.second, height_range.first, height_range.second, dev_out_f32, entries));
    }
    void resolve_varyings(void *dev_out_f32, uint64_t entries) { resolve_varyings(dev_out_f32, entries, {0, (int32_t)width_}, {0, (int32_t)height_}); }
    // the same on the host: `out` is resized to (y1 - y0) * x1 * K floats (new elements = fill, existing ones are kept: they are
    // what entries nobody owns hold afterwards); returns K, the varyings of the last geometry_processing / draw
    int readback_varyings(std::vector<float> &out, std::pair<int32_t, int32_t> width_range, std::pair<int32_t, int32_t> height_range, float fill = 0.0f)
    {
        const int num_varyings = frr_geometry_num_varyings(ctx_);   // the library's own K: the copy-back never passes `out`
        if (num_varyings < 0) throw Error(FRR_ERR_INVALID, "readback_varyings before geometry_processing");
        const int64_t rows = (int64_t)height_range.second - height_range.first;
        const uint64_t entries = rows > 0 && width_range.second > 0 ? (uint64_t)rows * (uint64_t)width_range.second : 0;
        out.resize((size_t)entries * (size_t)(num_varyings > 0 ? num_varyings : 0), fill);
        float none = fill;
        check(frr_readback_varyings(ctx_, width_range.first, width_range.second, height_range.first, height_range.second, out.empty() ? &none : out.data(), entries));
        return num_varyings > 0 ? num_varyings : 0;
    }
    int readback_varyings(std::vector<float> &out, float fill = 0.0f) { return readback_varyings(out, {0, (int32_t)width_}, {0, (int32_t)height_}, fill); }
    int geometry_num_varyings()
    {
        const int num_varyings = frr_geometry_num_varyings(ctx_);
        if (num_varyings < 0) throw Error(FRR_ERR_INVALID, "geometry_num_varyings before geometry_processing");
        return num_varyings;
    }
    // pixel_shader over a buffer of varyings, f32 [entries][K], into the colour target: every pixel of the window whose triangle
    // id is not 0xFFFFFFFF and satisfies id - id_first < id_count becomes vec4_to_u8_array(pixel_shader(uniforms, &in[i * K])),
    // i = (cy - y0) * x1 + (cx - x0); every other pixel, depth, ids and stats() are untouched (include/frr.h:
    // frr_shade_varyings).  Device memory that stays allocated and unchanged until sync or the next clear; no host wait.
    void shade_varyings(int pixel_shader, const void *dev_in_f32, uint64_t entries, int num_varyings, std::pair<int32_t, int32_t> width_range,
                        std::pair<int32_t, int32_t> height_range, uint32_t id_first = 0, uint32_t id_count = 0xFFFFFFFFu)
    {
        check(frr_shade_varyings(ctx_, pixel_shader, width_range.first, width_range.second, height_range.first, height_range.second, dev_in_f32, entries,
                                 num_varyings, id_first, id_count));
    }
    void shade_varyings(int pixel_shader, const void *dev_in_f32, uint64_t entries, int num_varyings, uint32_t id_first = 0, uint32_t id_count = 0xFFFFFFFFu)
    {
        shade_varyings(pixel_shader, dev_in_f32, entries, num_varyings, {0, (int32_t)width_}, {0, (int32_t)height_}, id_first, id_count);
    }
    // the same from host memory: `in` holds entries * K floats, entries = in.size() / K (K == 0: none are read); copied to the
    // device inside the call
    void shade_varyings_host(int pixel_shader, const std::vector<float> &in, int num_varyings, std::pair<int32_t, int32_t> width_range,
                             std::pair<int32_t, int32_t> height_range, uint32_t id_first = 0, uint32_t id_count = 0xFFFFFFFFu)
    {
        const int64_t rows = (int64_t)height_range.second - height_range.first;
        const uint64_t window = rows > 0 && width_range.second > 0 ? (uint64_t)rows * (uint64_t)width_range.second : 0;
        const uint64_t entries = num_varyings > 0 ? (uint64_t)in.size() / (uint64_t)num_varyings : window;
        check(frr_shade_varyings_host(ctx_, pixel_shader, width_range.first, width_range.second, height_range.first, height_range.second,
                                      in.empty() ? nullptr : in.data(), entries, num_varyings, id_first, id_count));
    }
    void shade_varyings_host(int pixel_shader, const std::vector<float> &in, int num_varyings, uint32_t id_first = 0, uint32_t id_count = 0xFFFFFFFFu)
    {
        shade_varyings_host(pixel_shader, in, num_varyings, {0, (int32_t)width_}, {0, (int32_t)height_}, id_first, id_count);
    }
    // shade_varyings for all the items of the latest geometry pass at once, each under its own material: what one ranged
    // shade_varyings per item of item_ranges() under that item's texture slot, strengths, flat colour and u.user[0 .. 8) leaves,
    // byte for byte, in one pass over the window (include/frr.h: frr_shade_items).  Everything else in the uniforms is the call's.
    void shade_items(int pixel_shader, const void *dev_in_f32, uint64_t entries, int num_varyings, const Materials &materials,
                     std::pair<int32_t, int32_t> width_range, std::pair<int32_t, int32_t> height_range)
    {
        check(frr_shade_items(ctx_, pixel_shader, width_range.first, width_range.second, height_range.first, height_range.second, dev_in_f32, entries,
                              num_varyings, materials.id));
    }
    void shade_items(int pixel_shader, const void *dev_in_f32, uint64_t entries, int num_varyings, const Materials &materials)
    {
        shade_items(pixel_shader, dev_in_f32, entries, num_varyings, materials, {0, (int32_t)width_}, {0, (int32_t)height_});
    }
    // the same from host memory, as shade_varyings_host takes it
    void shade_items_host(int pixel_shader, const std::vector<float> &in, int num_varyings, const Materials &materials,
                          std::pair<int32_t, int32_t> width_range, std::pair<int32_t, int32_t> height_range)
    {
        const int64_t rows = (int64_t)height_range.second - height_range.first;
        const uint64_t window = rows > 0 && width_range.second > 0 ? (uint64_t)rows * (uint64_t)width_range.second : 0;
        const uint64_t entries = num_varyings > 0 ? (uint64_t)in.size() / (uint64_t)num_varyings : window;
        check(frr_shade_items_host(ctx_, pixel_shader, width_range.first, width_range.second, height_range.first, height_range.second,
                                   in.empty() ? nullptr : in.data(), entries, num_varyings, materials.id));
    }
    void shade_items_host(int pixel_shader, const std::vector<float> &in, int num_varyings, const Materials &materials)
    {
        shade_items_host(pixel_shader, in, num_varyings, materials, {0, (int32_t)width_}, {0, (int32_t)height_});
    }
    frr_stats stats() { frr_stats s; check(frr_get_stats(ctx_, &s)); return s; }
    frr_ctx *raw() { return ctx_; }

private:
    // negative status: throw; a positive one (warning; none defined at present): results were delivered, remembered in last_warning
    void check(int rc) { if (rc < FRR_OK) throw Error(rc, frr_last_error(ctx_)); last_warning = rc; }
    // the host form of a count command (frr_visible_pixels_host, frr_query_pixels_host): n first, then the counts
    std::vector<uint32_t> counts_on_host(int (*host)(frr_ctx *, int, int32_t, int32_t, int32_t, int32_t, uint32_t *, uint64_t, uint64_t *), int unit,
                                         std::pair<int32_t, int32_t> wr, std::pair<int32_t, int32_t> hr)
    {
        uint64_t n = 0;
        uint32_t probe = 0;   // (one entry is enough to ask for n)
        check(host(ctx_, unit, wr.first, wr.second, hr.first, hr.second, &probe, 1, &n));
        std::vector<uint32_t> out((size_t)n, probe);
        if (n > 1) check(host(ctx_, unit, wr.first, wr.second, hr.first, hr.second, out.data(), n, &n));
        return out;
    }
public:
    int last_warning = FRR_OK;
private:
    frr_ctx *ctx_ = nullptr;
    uint32_t width_, height_;
};

} // namespace frr
