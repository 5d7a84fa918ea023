// update_scene_check — drives racc::updateScene (include/RayAccelerator.h): creates a scene from a mesh, refits it to a second vertex
// set, renders ONE set of rays through racc::render — a spawn callback hands them out, a shade callback copies the Results — and writes
// the Results, in the rays' order, to a file the Python side compares with the oracle on the host-refitted blobs.
//   update_scene_check <mesh.bin> <moved_vertices.bin> <rays.bin> <out.bin>
//     mesh.bin            {u32 vertexCount, u32 triangleCount} vertices[vertexCount] (xyzw f32) indices[3 * triangleCount] (u32)
//     moved_vertices.bin  vertices[vertexCount]
//     rays.bin            {u32 count} Ray[count];  out.bin: Result[count]
// RACC_FAST_TRAVERSAL=1: updateScene must refuse; the exit code is then 7 and nothing is rendered.
#include "RayAccelerator.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct App {
    std::vector<racc::Ray> rays;
    std::vector<racc::Result> results;
    std::vector<uint32_t> origin;                       // [stream][slot] -> index of the ray
    racc::ContextInfo info;
    unsigned perSpawn = 0;
    std::atomic<unsigned> next{0};
    std::atomic<unsigned> shaded{0};
};

bool spawn(void* data, unsigned, racc::RayStream* out) {
    App* app = static_cast<App*>(data);
    const unsigned total = unsigned(app->rays.size());
    const unsigned begin = app->next.fetch_add(app->perSpawn);
    if (begin >= total) return false;
    const unsigned end = begin + app->perSpawn < total ? begin + app->perSpawn : total;
    uint32_t* org = app->origin.data() + size_t(out->index) * app->info.rayStreamSize;
    for (unsigned i = begin; i < end; ++i) {
        out->rays[out->count] = app->rays[i];
        org[out->count] = i;
        ++out->count;
    }
    return end < total;
}

void shade(void* data, unsigned, const racc::RayStream* in, unsigned start, unsigned end, racc::RayStream*) {
    App* app = static_cast<App*>(data);
    const uint32_t* org = app->origin.data() + size_t(in->index) * app->info.rayStreamSize;
    for (unsigned i = start; i < end; ++i) app->results[org[i]] = in->results[i];
    app->shaded += end - start;
}

template <class T> bool readAll(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return std::fread(v.data(), sizeof(T), n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: update_scene_check mesh.bin moved_vertices.bin rays.bin out.bin\n"); return 2; }
    std::vector<racc::Vertex> vertices, moved;
    std::vector<uint32_t> indices;
    App app;
    {
        uint32_t head[2] = {0, 0}, count = 0;
        FILE* f = std::fopen(argv[1], "rb");
        bool ok = f && std::fread(head, 4, 2, f) == 2 && readAll(f, vertices, head[0]) && readAll(f, indices, size_t(head[1]) * 3);
        if (f) std::fclose(f);
        f = std::fopen(argv[2], "rb");
        ok = ok && f && readAll(f, moved, head[0]);
        if (f) std::fclose(f);
        f = std::fopen(argv[3], "rb");
        ok = ok && f && std::fread(&count, 4, 1, f) == 1 && readAll(f, app.rays, count);
        if (f) std::fclose(f);
        if (!ok) { std::fprintf(stderr, "update_scene_check: cannot read the inputs\n"); return 2; }
    }
    app.results.resize(app.rays.size());

    racc::init();
    racc::Configuration cfg = racc::defaultConfiguration(racc::gpuContextForDevice(0));
    if (const char* t = std::getenv("RACC_CPU_THREADS")) cfg.cpuThreads = unsigned(std::atoi(t));
    racc::Context* ctx = racc::createContext(cfg);
    if (!ctx) return 3;
    app.info = racc::info(ctx);
    app.perSpawn = cfg.maxRaysPerSpawn;
    app.origin.resize(size_t(app.info.rayStreamCount) * app.info.rayStreamSize);
    racc::Scene* scene = racc::createScene(ctx, vertices.data(), unsigned(vertices.size()), indices.data(), unsigned(indices.size()));
    if (!scene) return 3;
    if (!racc::updateScene(scene, moved.data(), unsigned(moved.size()))) {
        racc::destroy(scene); racc::destroy(ctx); racc::deinit();
        return 7;
    }
    racc::RenderCallbacks cb = { &app, spawn, shade };
    const racc::Stats stats = racc::render(ctx, scene, nullptr, cb);
    if (const char* err = racc::lastError(ctx)) { std::fprintf(stderr, "update_scene_check: %s\n", err); return 5; }
    FILE* o = std::fopen(argv[4], "wb");
    if (!o) return 2;
    std::fwrite(app.results.data(), sizeof(racc::Result), app.results.size(), o);
    std::fclose(o);
    std::printf("{\"raysTraced\": %llu, \"shaded\": %u}\n", (unsigned long long)stats.raysTraced, app.shaded.load());
    racc::destroy(scene); racc::destroy(ctx); racc::deinit();
    return stats.raysTraced == app.rays.size() && app.shaded.load() == app.rays.size() ? 0 : 4;
}
