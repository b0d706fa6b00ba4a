// phong_headless.cpp -- headless equivalent of /root/reference/examples/src/bin/phong.rs:314-387
// on the C++ host mirror: clear -> per mesh { geometry_processing ; rasterization } -> get_data,
// with the window/Vulkan presentation (out of scope) replaced by a raw RGBA dump and a PPM.
//
//   phong_headless <mesh.f32> <ntris> <tex.rgba> <tex_size> <W> <H> <out.rgba> [<out.ppm>]
//       mesh.f32: ntris x 3 x 8 float32 (pos3, uv2, normal3 = VSInput, phong.rs:49-54)
//   phong_headless --assets <model.obj> <diffuse.tga> <W> <H> <out.rgba> [<out.ppm>]
//       the reference's own asset formats: Model::new (obj_loader.rs:15-97), uploaded as an indexed mesh (the expansion of
//       init_vertex_input, phong.rs:187-201, is the GPU's gather)
//       and FrameBuffer::load_file (renderer.rs:427-471, BGRA storage)
//   a --wireframe anywhere among the arguments of the two forms above overlays the mesh's edges (FrameBuffer::draw_line,
//       renderer.rs:540-588, over the setup triangles) in white after the shaded draw, on the device
//   a --deferred anywhere among them shades the frame in a pass of its own: a depth-only pre-pass (FRR_PS_DEPTH), the pixel
//       shader's input of every pixel's final owner read back (readback_varyings), and FRR_PS_PHONG run over that buffer
//       (shade_varyings_host) -- the same bytes as the forward run
//   --instances N anywhere among them draws the mesh N times, on a grid of translations (scaled down to fit), with ONE call:
//       the loop over objects of phong.rs:319-331 as one instanced pass (draw_instanced)
//   --list anywhere among them draws the objects -- the N copies of --instances, else the one mesh -- as (mesh, model matrix) items
//       of ONE list pass (draw_list): the setup loop of phong.rs:319-359, where every object may name a mesh of its own
//   --visible with --list or --instances N prints, after the draw, one line per item -- its first triangle id, the triangles
//       it emitted and the pixels it owns on screen (visible_pixels: counted on the device, the frame is not read back for
//       it) -- and the number of items that own no pixel; the frame written is the same
//   --reuse with --list --visible draws a SECOND frame from the first one's counts: the counts go to device memory
//       (visible_pixels), and after clear the list is drawn again with draw_list_if on that buffer -- an item that owned no
//       pixel is dropped -- with no host wait between the count and the draw; it prints how many items the second frame dropped
//       and whether its colour equals the first frame's.  (The mechanism only: an item that was hidden stays dropped until the
//       caller's own policy sets its entry again.)
//   --materials with --list --deferred gives every object a material of its own -- texture slots 0, 1, 2 in turn (the diffuse
//       texture, and it with its first / its second channel inverted) and a flat colour in turn -- and shades the whole list
//       with ONE pass over the frame (shade_items_host): phong.rs:361-370, a ps_uniform per object, for a list
//   --boxes with --list runs the loop of --occlusion with the box query in the proxy pass's place: the objects' bounds computed on
//       the device (list_bounds), their boxes tested against a pyramid of the occluder's depth (query_boxes: no geometry pass, no
//       binning), the objects it keeps drawn (draw_list_if).  It prints per item the status and the value, and whether colour and
//       depth equal the frame that draws every object
//   --occlusion with --list draws the mesh once more, unscaled, as an occluder in front of the right part of the grid, and then
//       runs the occlusion loop of INTEGRATION.md 1f with no host wait in between: the objects' bounding boxes as a proxy list,
//       queried against the occluder's depth (query_pixels: nothing is drawn), the objects whose box passed somewhere drawn
//       (draw_list_if on the counts), what ended up on screen counted (visible_pixels).  It prints per item the proxy's count,
//       the object's own count and its visible pixels, how many items were skipped, and whether colour and depth equal the
//       frame that draws every object
//   --cull neg|pos anywhere among them drops the input triangles whose clip-space determinant is negative / positive before
//       they are set up (set_cull): on a closed mesh, the faces that look away from the camera
//   phong_headless --dump-assets <model.obj> <diffuse.tga> <mesh_out.f32> <tex_out.rgba>
//       loaders only (no GPU): what the two loaders produce, for the CPU-side check against the Python mirror
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "../f_renderer_amd/host/frr_renderer.hpp"

// --reuse: one device buffer of the HIP runtime libfrr_hip.so itself runs on (no HIP header is needed for three calls)
extern "C" int hipMalloc(void **ptr, size_t size);
extern "C" int hipFree(void *ptr);
extern "C" int hipMemcpy(void *dst, const void *src, size_t size, int kind);

static std::vector<char> slurp(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) { std::cerr << "cannot open " << path << "\n"; std::exit(2); }
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv)
{
    bool wireframe = false, deferred = false, list = false, visible = false, reuse = false, materials = false, occlusion = false, boxes = false;
    for (int i = 1; i < argc; ++i)
        if (std::string(argv[i]) == "--wireframe" || std::string(argv[i]) == "--deferred" || std::string(argv[i]) == "--list" || std::string(argv[i]) == "--visible" || std::string(argv[i]) == "--reuse" ||
            std::string(argv[i]) == "--materials" || std::string(argv[i]) == "--occlusion" || std::string(argv[i]) == "--boxes") {
            (std::string(argv[i]) == "--wireframe" ? wireframe : std::string(argv[i]) == "--list" ? list : std::string(argv[i]) == "--visible" ? visible : std::string(argv[i]) == "--reuse" ? reuse :
             std::string(argv[i]) == "--materials" ? materials : std::string(argv[i]) == "--occlusion" ? occlusion : std::string(argv[i]) == "--boxes" ? boxes : deferred) = true;
            for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
            --argc; --i;
        }
    long instances = -1;
    for (int i = 1; i + 1 < argc; ++i)
        if (std::string(argv[i]) == "--instances") {
            instances = std::atol(argv[i + 1]);
            for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
            argc -= 2; --i;
        }
    int cull = FRR_CULL_NONE;
    for (int i = 1; i + 1 < argc; ++i)
        if (std::string(argv[i]) == "--cull") {
            const std::string v = argv[i + 1];
            if (v != "neg" && v != "pos") { std::cerr << "--cull takes neg or pos\n"; return 2; }
            cull = v == "neg" ? FRR_CULL_NEG : FRR_CULL_POS;
            for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
            argc -= 2; --i;
        }
    if (visible && !list && instances < 0) { std::cerr << "--visible goes with --list or --instances N\n"; return 2; }
    if (reuse && (!list || !visible || wireframe || deferred)) { std::cerr << "--reuse goes with --list --visible (and without --wireframe / --deferred)\n"; return 2; }
    if (materials && (!list || !deferred)) { std::cerr << "--materials goes with --list --deferred\n"; return 2; }
    if (boxes && (!list || occlusion || visible || reuse || wireframe || deferred)) { std::cerr << "--boxes goes with --list (and without --occlusion / --visible / --reuse / --wireframe / --deferred)\n"; return 2; }
    if (occlusion && (!list || visible || reuse || wireframe || deferred)) { std::cerr << "--occlusion goes with --list (and without --visible / --reuse / --wireframe / --deferred)\n"; return 2; }
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "--dump-assets") {
        if (argc < 6) { std::cerr << "usage: phong_headless --dump-assets model.obj diffuse.tga mesh_out.f32 tex_out.rgba\n"; return 2; }
        try {
            const frr::Model model(argv[2]);
            const auto vin = model.vertex_inputs();
            const frr::FrameBuffer tex = frr::FrameBuffer::load_file(argv[3]);
            std::ofstream(argv[4], std::ios::binary).write(reinterpret_cast<const char *>(vin.data()), (std::streamsize)(vin.size() * sizeof(vin[0])));
            std::ofstream(argv[5], std::ios::binary).write(reinterpret_cast<const char *>(tex.get_data().data()), tex.get_size());
            std::printf("faces=%zu tex=%ux%u\n", model.faces_len(), tex.width(), tex.height());
        } catch (const frr::Error &e) { std::cerr << e.what() << "\n"; return 1; }
        return 0;
    }
    const bool assets = mode == "--assets";
    if ((assets && argc < 7) || (!assets && argc < 8)) {
        std::cerr << "usage: phong_headless mesh.f32 ntris tex.rgba tex_size W H out.rgba [out.ppm]\n"
                     "       phong_headless --assets model.obj diffuse.tga W H out.rgba [out.ppm]\n"
                     "       (--wireframe: overlay the mesh's edges; --deferred: depth pre-pass, varyings, shade;\n"
                     "        --instances N: N copies on a grid in one instanced pass; --list: the objects as one list pass;\n"
                     "        --cull neg|pos: drop the inputs whose clip-space determinant has that sign;\n"
                     "        --visible (with --list or --instances N): print the pixels every item owns on screen;\n"
                     "        --reuse (with --list --visible): a second frame by draw_list_if on the first one's counts;\n"
                     "        --materials (with --list --deferred): a texture slot and a flat colour per object, one shade_items;\n"
                     "        --occlusion (with --list): an occluder in front of part of the list, box proxies queried against its depth\n"
                     "        (query_pixels), and only the objects whose proxy passed drawn (draw_list_if);\n"
                     "        --boxes (with --list): the same occluder, the objects' bounds computed on the device (list_bounds), their boxes\n"
                     "        tested against the depth pyramid (query_boxes: no proxy pass), and only the objects it keeps drawn)\n";
        return 2;
    }
    const int a0 = assets ? 4 : 5;                                             // index of W
    const uint32_t W = (uint32_t)std::atoi(argv[a0]), H = (uint32_t)std::atoi(argv[a0 + 1]);
    const char *out_rgba = argv[a0 + 2], *out_ppm = argc > a0 + 3 ? argv[a0 + 3] : nullptr;
    try {
        std::vector<std::array<frr::VSInput, 3>> vin;
        frr::Model::Indexed indexed;                                          // --assets: the Model as it is, not expanded
        frr::FrameBuffer diffuse(1, 1);
        if (assets) {
            indexed = frr::Model(argv[2]).indexed_inputs();                   // phong.rs:166; :187-201 happens on the GPU
            diffuse = frr::FrameBuffer::load_file(argv[3]);                   // phong.rs:167
        } else {
            const uint64_t ntris = std::strtoull(argv[2], nullptr, 10);
            const uint32_t ts = (uint32_t)std::atoi(argv[4]);
            const auto mesh_bytes = slurp(argv[1]);
            const auto tex_bytes = slurp(argv[3]);
            if (mesh_bytes.size() != ntris * 96 || tex_bytes.size() != (size_t)ts * ts * 4) { std::cerr << "size mismatch\n"; return 2; }
            vin.resize(ntris);
            std::memcpy(vin.data(), mesh_bytes.data(), mesh_bytes.size());
            diffuse = frr::FrameBuffer(ts, ts);                               // FrameBuffer::load_file stand-in
            std::memcpy(diffuse.get_data_mut().data(), tex_bytes.data(), tex_bytes.size());
        }

        frr::Renderer renderer(W, H);
        renderer.set_texture(0, diffuse);

        frr::Camera camera_1({0.0f, 1.0f, 3.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f});       // phong.rs:158-162 (at: SURVEY 8d)
        const frr::Mat4 proj = frr::set_perspective(3.14159274101257324f * 0.25f, (float)W / (float)H, 0.1f, 100.0f); // phong.rs:164
        const frr::Mat4 model = frr::set_identity();                                            // phong.rs:156
        std::memcpy(renderer.uniforms.model, model.data(), 64);
        std::memcpy(renderer.uniforms.view, camera_1.mat_look_at.data(), 64);
        std::memcpy(renderer.uniforms.proj, proj.data(), 64);
        renderer.uniforms.view_pos[0] = camera_1.eye.x; renderer.uniforms.view_pos[1] = camera_1.eye.y; renderer.uniforms.view_pos[2] = camera_1.eye.z;
        renderer.uniforms.texture_slot = 0;                                                     // PSUniform.place
        renderer.set_uniforms();

        frr::Mesh mesh = assets ? renderer.upload_mesh_indexed(indexed, FRR_VS_PHONG) : renderer.upload_mesh(vin, FRR_VS_PHONG);
        if (assets) std::printf("indexed: nverts=%zu ntris=%zu\n", indexed.vertices.size(), indexed.faces.size());
        frr::FrameBuffer frame_buffer = frr::FrameBuffer::create(W, H);                         // phong.rs:207

        renderer.clear({30, 30, 30, 255}, 0.0f);                                                // phong.rs:316-317
        if (cull != FRR_CULL_NONE) renderer.set_cull(cull);
        std::vector<frr::Mat4> models;
        if (instances >= 0) {
            // N objects that share the mesh: model_i = translate(grid cell i) * scale(1 / columns), column-major
            const long cols = std::max(1L, (long)std::ceil(std::sqrt((double)std::max(instances, 1L))));
            const float s = 1.0f / (float)cols;
            models.assign((size_t)instances, frr::set_identity());
            for (long i = 0; i < instances; ++i) {
                frr::Mat4 &m = models[(size_t)i];
                m[0] = m[5] = m[10] = s;
                m[12] = (((float)(i % cols) + 0.5f) * s - 0.5f) * 3.0f;
                m[13] = (((float)(i / cols) + 0.5f) * s - 0.5f) * 2.0f;
                m[14] = -0.25f * (float)(i % 3);
            }
        } else if (list) models.assign(1, model);
        if (boxes) {
            // The loop of --occlusion without the proxy pass: the occluder, then -- no host wait in between -- query_boxes over the
            // objects' own list (bounds from list_bounds: nothing of the mesh is read on the host) and draw_list_if on its answer.
            const uint64_t n = models.size();
            const frr::DrawList objects = renderer.upload_draw_list(std::vector<frr::Mesh>((size_t)n, mesh), models);
            std::vector<float> lo_hi; std::vector<uint32_t> flags;
            renderer.list_bounds(objects, lo_hi, flags);                                        // on the device, once per distinct mesh
            frr::Mat4 occluder = frr::set_identity();
            occluder[12] = 0.9f; occluder[13] = -0.1f; occluder[14] = 1.0f;
            auto draw_occluder = [&] {
                std::memcpy(renderer.uniforms.model, occluder.data(), 64); renderer.set_uniforms();
                renderer.draw(mesh, FRR_PS_PHONG);
                std::memcpy(renderer.uniforms.model, model.data(), 64); renderer.set_uniforms();
            };
            frr::FrameBuffer all = frr::FrameBuffer::create(W, H);
            std::vector<float> all_depth, depth, occ_depth;
            draw_occluder();
            renderer.read_depth(occ_depth);                                                     // (for the host build of the rule, below)
            renderer.draw_list(objects, FRR_PS_PHONG);                                          // the frame that draws everything
            renderer.read_frame_buffer(all);
            renderer.read_depth(all_depth);
            uint32_t *dev = nullptr;
            if (hipMalloc((void **)&dev, (size_t)(n ? n : 1) * 2 * sizeof(uint32_t)) != 0) { std::cerr << "hipMalloc failed\n"; return 1; }
            renderer.clear({30, 30, 30, 255}, 0.0f);
            draw_occluder();
            renderer.query_boxes(objects, dev, n);                                              // can the object change a pixel of what is there?
            renderer.draw_list_if(objects, dev, n, FRR_PS_PHONG);                               // keep[i] >= 1
            renderer.visible_pixels(FRR_PER_ITEM, dev + n, n);
            renderer.read_frame_buffer(frame_buffer);                                           // (the first host wait of the loop)
            renderer.read_depth(depth);
            std::vector<uint32_t> host((size_t)n * 2, 0u), rule((size_t)n, 0u);
            if (n && hipMemcpy(host.data(), dev, host.size() * sizeof(uint32_t), 2 /* device to host */) != 0) { std::cerr << "hipMemcpy failed\n"; return 1; }
            // the status of every item, by the host build of the rule over the occluder's depth: the values have to be the device's
            std::vector<float> mvps((size_t)n * 16);
            std::vector<int32_t> srl((size_t)n * 6, 0);
            for (size_t k = 0; k < (size_t)n; ++k) frr_host_instance_mvp(renderer.uniforms.proj, renderer.uniforms.view, models[k].data(), &mvps[16 * k]);
            if (frr_host_query_boxes(mvps.data(), lo_hi.data(), flags.data(), n, W, H, 0, (int32_t)W, 0, (int32_t)H, occ_depth.data(), occ_depth.size(), nullptr,
                                     rule.data(), n, srl.data()) != (int64_t)n) { std::cerr << "frr_host_query_boxes failed\n"; return 1; }
            static const char *const names[5] = {"none", "outside", "hidden", "kept", "unbounded"};
            size_t skipped = 0;
            for (size_t k = 0; k < (size_t)n; ++k) {
                std::printf("item %zu: %s, value %u, visible pixels %u\n", k, names[srl[6 * k]], host[k], host[(size_t)n + k]);
                skipped += host[k] == 0u;
                if (host[k] != rule[k]) { std::cerr << "item " << k << ": the device's value differs from the host build's\n"; return 3; }
                if (host[(size_t)n + k] > host[k]) { std::cerr << "item " << k << ": owns more pixels than the query promised\n"; return 3; }
            }
            const bool same_colour = frame_buffer.get_data() == all.get_data();
            const bool same_depth = depth.size() == all_depth.size() && std::memcmp(depth.data(), all_depth.data(), depth.size() * sizeof(float)) == 0;
            std::printf("boxes: skipped %zu of %zu items, colour equal: %s, depth equal: %s\n", skipped, (size_t)n, same_colour ? "yes" : "no", same_depth ? "yes" : "no");
            (void)hipFree(dev);
            std::ofstream(out_rgba, std::ios::binary).write(reinterpret_cast<const char *>(frame_buffer.get_data().data()), frame_buffer.get_size());
            return 0;
        }
        if (occlusion) {
            // An occluder in front of part of the list; then, with no host wait in between: the box proxies of all objects queried
            // against its depth, the objects whose proxy passed drawn, what ended up on screen counted (with
            // nothing known from a frame before).  The frame must equal the one that draws every object.
            const uint64_t n = models.size();
            float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
            auto grow = [&](const frr::VSInput &v) { for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], v.pos[k]); hi[k] = std::max(hi[k], v.pos[k]); } };
            for (const auto &t : vin) for (const auto &v : t) grow(v);
            for (const auto &v : indexed.vertices) grow(v);
            const float inflate = 0.02f;   // about a pixel's worth: the box is conservative only up to the snap to integer pixels
            for (int k = 0; k < 3; ++k) { lo[k] -= inflate; hi[k] += inflate; }
            static const int quads[6][4] = {{0, 1, 3, 2}, {4, 6, 7, 5}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 5, 7, 3}};   // corner i: bit k picks hi
            std::vector<std::array<frr::VSInput, 3>> box(12);
            std::memset(box.data(), 0, box.size() * sizeof(box[0]));
            for (int q = 0; q < 6; ++q)
                for (int h = 0; h < 2; ++h)
                    for (int v = 0; v < 3; ++v) {
                        const int corner = quads[q][h == 0 ? v : (v == 0 ? 0 : v + 1)];
                        for (int k = 0; k < 3; ++k) box[(size_t)(2 * q + h)][(size_t)v].pos[k] = (corner >> k) & 1 ? hi[k] : lo[k];
                    }
            const frr::Mesh box_mesh = renderer.upload_mesh(box, FRR_VS_PHONG);
            const frr::DrawList objects = renderer.upload_draw_list(std::vector<frr::Mesh>((size_t)n, mesh), models);
            const frr::DrawList proxies = renderer.upload_draw_list(std::vector<frr::Mesh>((size_t)n, box_mesh), models);
            frr::Mat4 occluder = frr::set_identity();
            occluder[12] = 0.9f; occluder[13] = -0.1f; occluder[14] = 1.0f;   // the mesh itself, unscaled, in front of the right part of the grid
            auto draw_occluder = [&] {
                std::memcpy(renderer.uniforms.model, occluder.data(), 64); renderer.set_uniforms();
                renderer.draw(mesh, FRR_PS_PHONG);
                std::memcpy(renderer.uniforms.model, model.data(), 64); renderer.set_uniforms();
            };
            frr::FrameBuffer all = frr::FrameBuffer::create(W, H);
            std::vector<float> all_depth, depth;
            draw_occluder();
            renderer.draw_list(objects, FRR_PS_PHONG);                                          // the frame that draws everything
            renderer.read_frame_buffer(all);
            renderer.read_depth(all_depth);
            uint32_t *dev = nullptr;
            if (hipMalloc((void **)&dev, (size_t)(n ? n : 1) * 3 * sizeof(uint32_t)) != 0) { std::cerr << "hipMalloc failed\n"; return 1; }
            uint32_t *q_box = dev, *q_own = dev + n, *vis = dev + 2 * n;
            renderer.clear({30, 30, 30, 255}, 0.0f);
            draw_occluder();
            renderer.geometry_list(proxies);
            renderer.query_pixels(FRR_PER_ITEM, q_box, n);                                      // would the box be visible against what is there?
            renderer.geometry_list(objects);
            renderer.query_pixels(FRR_PER_ITEM, q_own, n);                                      // (the objects themselves, for the print below)
            renderer.draw_list_if(objects, q_box, n, FRR_PS_PHONG);                             // keep[i] >= 1: the proxy passed somewhere
            renderer.visible_pixels(FRR_PER_ITEM, vis, n);
            renderer.read_frame_buffer(frame_buffer);                                           // (the first host wait of the loop)
            renderer.read_depth(depth);
            std::vector<uint32_t> host((size_t)n * 3, 0u);
            if (n && hipMemcpy(host.data(), dev, host.size() * sizeof(uint32_t), 2 /* device to host */) != 0) { std::cerr << "hipMemcpy failed\n"; return 1; }
            size_t skipped = 0;
            for (size_t k = 0; k < (size_t)n; ++k) {
                std::printf("item %zu: proxy count %u, own count %u, visible pixels %u\n", k, host[k], host[(size_t)n + k], host[2 * (size_t)n + k]);
                skipped += host[k] == 0u;
                if (host[k] == 0u && host[(size_t)n + k] != 0u) { std::cerr << "item " << k << ": its proxy is hidden, the object is not\n"; return 3; }
            }
            const bool same_colour = frame_buffer.get_data() == all.get_data();
            const bool same_depth = depth.size() == all_depth.size() && std::memcmp(depth.data(), all_depth.data(), depth.size() * sizeof(float)) == 0;
            std::printf("occlusion: skipped %zu of %zu items, colour equal: %s, depth equal: %s\n", skipped, (size_t)n, same_colour ? "yes" : "no", same_depth ? "yes" : "no");
            (void)hipFree(dev);
            std::ofstream(out_rgba, std::ios::binary).write(reinterpret_cast<const char *>(frame_buffer.get_data().data()), frame_buffer.get_size());
            return 0;
        }
        frr::DrawList items;
        if (list) {
            items = renderer.upload_draw_list(std::vector<frr::Mesh>(models.size(), mesh), models);
            renderer.geometry_list(items);                                                      // loop A for every item, one pass
            std::vector<uint32_t> first, count;
            renderer.item_ranges(first, count);                                                 // body_offset, face_offset, ... (phong.rs:333-359)
            std::printf("list: n=%zu tris_in=%llu last_first=%u\n", models.size(), (unsigned long long)renderer.stats().tris_in, first.empty() ? 0u : first.back());
        } else if (instances >= 0) {
            const frr::Instances table = renderer.upload_instances(models);
            renderer.geometry_processing_instanced(mesh, table);                                // loop A for every object, one pass
            std::printf("instances: n=%ld tris_in=%llu\n", instances, (unsigned long long)renderer.stats().tris_in);
        } else
        renderer.geometry_processing(mesh);                                                     // loop A
        if (!deferred) {
            renderer.rasterization({0, (int32_t)W}, {0, (int32_t)H}, FRR_PS_PHONG);             // loop B
        } else {
            renderer.rasterization({0, (int32_t)W}, {0, (int32_t)H}, FRR_PS_DEPTH);             // loop B without renderer.rs:380-381 ...
            std::vector<float> varyings;
            const int num_varyings = renderer.readback_varyings(varyings);                      // ... its `input` (:368-378) per pixel ...
            if (!materials) renderer.shade_varyings_host(FRR_PS_PHONG, varyings, num_varyings); // ... and :380-381 over that buffer
            else {
                // ... under a ps_uniform per object (phong.rs:34-47, 361-370): slots 1 and 2 hold the diffuse texture with its
                // first / second channel inverted, object k samples slot k % 3; one pass over the frame for all of them
                for (int slot = 1; slot <= 2; ++slot) {
                    frr::FrameBuffer t = diffuse;
                    for (size_t i = (size_t)slot - 1; i < t.get_data_mut().size(); i += 4) t.get_data_mut()[i] = (uint8_t)(255 - t.get_data_mut()[i]);
                    renderer.set_texture(slot, t);
                }
                std::vector<frr_material> mats(models.size());
                for (size_t k = 0; k < mats.size(); ++k) {
                    frr_material &m = mats[k];
                    std::memset(&m, 0, sizeof m);
                    m.texture_slot = (int32_t)(k % 3);
                    m.ambient_strength = renderer.uniforms.ambient_strength; m.specular_strength = renderer.uniforms.specular_strength;
                    for (int ch = 0; ch < 3; ++ch) m.flat_color[ch] = (float)((k + (size_t)ch) % 4) / 3.0f;
                    m.flat_color[3] = 1.0f;
                }
                frr::Materials table = renderer.upload_materials(mats);
                renderer.shade_items_host(FRR_PS_PHONG, varyings, num_varyings, table);
                renderer.free_materials(table);                                                 // (finishes the shade first)
                std::printf("materials: n=%zu\n", mats.size());
            }
        }
        if (visible) {
            // which objects ended up on screen: the id target counted per item on the device (the wireframe and the shade pass
            // write colour only, so the place behind the raster pass is as good as any)
            const std::vector<uint32_t> pixels = renderer.visible_pixels(FRR_PER_ITEM);
            std::vector<uint32_t> first, count;
            renderer.item_ranges(first, count);
            size_t hidden = 0;
            for (size_t k = 0; k < pixels.size(); ++k) {
                std::printf("item %zu: first id %u, triangles %u, visible pixels %u\n", k, first[k], count[k], pixels[k]);
                hidden += pixels[k] == 0u;
            }
            std::printf("items that own no pixel: %zu of %zu\n", hidden, pixels.size());
        }
        if (wireframe) renderer.draw_wireframe({255, 255, 255, 255});                           // the edges over the shaded frame
        renderer.read_frame_buffer(frame_buffer);                                               // phong.rs:386

        const frr_stats st = renderer.stats();
        std::printf("tris_in=%llu tris_setup=%llu frag_covered=%llu\n", (unsigned long long)st.tris_in,
                    (unsigned long long)st.tris_setup, (unsigned long long)st.frag_covered);
        std::ofstream(out_rgba, std::ios::binary).write(reinterpret_cast<const char *>(frame_buffer.get_data().data()), frame_buffer.get_size());
        if (out_ppm) {
            std::ofstream ppm(out_ppm, std::ios::binary);
            ppm << "P6\n" << W << " " << H << "\n255\n";
            for (uint32_t i = 0; i < W * H; ++i) ppm.write(reinterpret_cast<const char *>(&frame_buffer.get_data()[(size_t)i * 4]), 3);
        }
        if (reuse) {
            // draw, count, draw again: the counts of the frame above stay on the device and decide what the next frame draws
            const uint64_t n = models.size();
            void *counts = nullptr;
            if (hipMalloc(&counts, (size_t)(n ? n : 1) * sizeof(uint32_t)) != 0) { std::cerr << "hipMalloc failed\n"; return 1; }
            renderer.visible_pixels(FRR_PER_ITEM, counts, n);                                   // per item of the list pass above
            renderer.clear({30, 30, 30, 255}, 0.0f);
            renderer.draw_list_if(items, counts, n, FRR_PS_PHONG);                              // keep[i] >= 1: the item owned a pixel
            frr::FrameBuffer second = frr::FrameBuffer::create(W, H);
            renderer.read_frame_buffer(second);                                                 // (the first host wait since the count)
            std::vector<uint32_t> host((size_t)n, 0u), first, count;
            if (n && hipMemcpy(host.data(), counts, (size_t)n * sizeof(uint32_t), 2 /* device to host */) != 0) { std::cerr << "hipMemcpy failed\n"; return 1; }
            renderer.item_ranges(first, count);
            size_t dropped = 0;
            for (size_t k = 0; k < (size_t)n; ++k) {
                dropped += host[k] == 0u;
                if ((host[k] == 0u) != (count[k] == 0u)) { std::cerr << "item " << k << ": dropped and emitting disagree\n"; return 3; }
            }
            const bool same = second.get_data() == frame_buffer.get_data();
            std::printf("reuse: dropped %zu of %zu items, colour equal: %s\n", dropped, (size_t)n, same ? "yes" : "no");
            (void)hipFree(counts);
        }
        // error behaviour: a range with min > max panics in the reference (i32::clamp) -> frr::Error here
        bool threw = false;
        try { renderer.rasterization({10, 5}, {0, (int32_t)H}, FRR_PS_PHONG); } catch (const frr::Error &e) { threw = e.code == FRR_ERR_INVALID; }
        if (!threw) { std::cerr << "expected FRR_ERR_INVALID\n"; return 3; }
    } catch (const frr::Error &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    return 0;
}
