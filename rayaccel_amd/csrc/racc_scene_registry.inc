// racc_scene_registry.inc — the public racc_hip_scene_upload / racc_hip_scene_free and the one record the library keeps per scene uploaded
// through them.  Textually included by racc_hip_unit.hip directly BEHIND racc_hip.hip, whose own upload / free are compiled under internal
// names (raccSceneUploadBase / raccSceneFreeBase, not exported: racc_hip.map) and wrapped here, once; racc_hip.hip itself is unchanged and
// racc_hip_scene gets no field.  A record holds the context the scene was uploaded on (racc_hip_world_create refuses another context's
// scene) and the blob's topology words, which a refit needs and the device does not hold: 16 B of host memory per inner node on EVERY
// upload, refitted or not (battlefield-synth: 17 MB), which RACC_REFIT_TOPOLOGY=0 switches off for a process that never refits.
// Scenes of a device group are uploaded by racc_group.inc inside racc_hip.hip, i.e. without a record: refit and instancing refuse them.

#include <unordered_map>

namespace {

struct RefitTopology { std::vector<uint32_t> words; uint32_t nodeCount = 0; };      // 4 per node: kind, parent, first, last

struct SceneRecord {
    const racc_hip_ctx* owner;
    std::shared_ptr<const RefitTopology> topology;      // may be null
    bool wideRefit = false;                             // a racc_hip_refit_create_wide handle exists (at most one per scene)
    // racc_hip_scene_rebuild_create made this scene (racc_scene_rebuild.inc): its records are in the rebuild's own layout, the topology words
    // are dropped for good (a device rebuild would make them stale) and the rebuild's handle is the scene's only handle ...
    bool rebuilt = false;
    bool rebuildLive = false;                           // ... which is alive: racc_hip_scene_free refuses
};

std::mutex g_sceneMutex;
std::unordered_map<const racc_hip_scene*, SceneRecord> g_scenes;

// the two lookups: null for a scene without a record (or, sceneTopology, without kept words)
std::shared_ptr<const RefitTopology> sceneTopology(const racc_hip_scene* scene) {
    std::lock_guard<std::mutex> g(g_sceneMutex);
    const auto it = g_scenes.find(scene);
    return it == g_scenes.end() ? nullptr : it->second.topology;
}

const racc_hip_ctx* sceneOwner(const racc_hip_scene* scene) {
    std::lock_guard<std::mutex> g(g_sceneMutex);
    const auto it = g_scenes.find(scene);
    return it == g_scenes.end() ? nullptr : it->second.owner;
}

// the one wide refit handle a scene may have: false when the scene has no record or the handle is already out; the release is the handle's destroy
bool sceneClaimWideRefit(const racc_hip_scene* scene) {
    std::lock_guard<std::mutex> g(g_sceneMutex);
    const auto it = g_scenes.find(scene);
    if (it == g_scenes.end() || it->second.wideRefit) return false;
    it->second.wideRefit = true;
    return true;
}

void sceneReleaseWideRefit(const racc_hip_scene* scene) {
    std::lock_guard<std::mutex> g(g_sceneMutex);
    const auto it = g_scenes.find(scene);
    if (it != g_scenes.end()) it->second.wideRefit = false;
}

// racc_hip_scene_rebuild_create: false for a scene without a record; the handle's destroy ends `rebuildLive`, `rebuilt` stays
bool sceneClaimRebuild(const racc_hip_scene* scene) {
    std::lock_guard<std::mutex> g(g_sceneMutex);
    const auto it = g_scenes.find(scene);
    if (it == g_scenes.end()) return false;
    it->second.topology.reset();
    it->second.rebuilt = it->second.rebuildLive = true;
    return true;
}

void sceneReleaseRebuild(const racc_hip_scene* scene) {
    std::lock_guard<std::mutex> g(g_sceneMutex);
    const auto it = g_scenes.find(scene);
    if (it != g_scenes.end()) it->second.rebuildLive = false;
}

bool sceneIsRebuilt(const racc_hip_scene* scene) {
    std::lock_guard<std::mutex> g(g_sceneMutex);
    const auto it = g_scenes.find(scene);
    return it != g_scenes.end() && it->second.rebuilt;
}

}  // namespace

extern "C" {

int racc_hip_scene_upload(racc_hip_ctx* ctx, const void* nodes64, uint32_t node_count, const void* pairs48, uint32_t pair_count,
                          const uint32_t* remap, uint32_t remap_count, racc_hip_scene** out) {
    if (int rc = raccSceneUploadBase(ctx, nodes64, node_count, pairs48, pair_count, remap, remap_count, out)) return rc;
    static const bool keepTopology = [] { const char* e = std::getenv("RACC_REFIT_TOPOLOGY"); return !e || std::atoi(e) != 0; }();
    // A bad_alloc below leaves the upload valid: the scene traces.  Without its topology it only cannot be refitted, without its record
    // it cannot become an instance either (racc_hip_refit_create / racc_hip_world_create say so).
    std::shared_ptr<RefitTopology> topo;
    if (keepTopology) try {
        topo = std::make_shared<RefitTopology>();
        topo->nodeCount = node_count;
        topo->words.resize(size_t(node_count) * 4);
        for (uint32_t i = 0; i < node_count; ++i) std::memcpy(&topo->words[size_t(i) * 4], static_cast<const char*>(nodes64) + size_t(i) * 64, 16);
    } catch (const std::bad_alloc&) {
        topo.reset();
    }
    try {
        std::lock_guard<std::mutex> g(g_sceneMutex);
        g_scenes[*out] = SceneRecord{ctx, std::move(topo)};
    } catch (const std::bad_alloc&) {
    }
    return RACC_HIP_OK;
}

int racc_hip_scene_free(racc_hip_ctx* ctx, racc_hip_scene* scene) {
    if (scene) {
        std::lock_guard<std::mutex> g(g_sceneMutex);
        const auto it = g_scenes.find(scene);
        if (it != g_scenes.end() && it->second.rebuildLive)
            return fail(RACC_HIP_ERR_INVALID, "scene_free: the scene has a rebuild handle (racc_hip_scene_rebuild_create): racc_hip_refit_destroy comes first");
        g_scenes.erase(scene);
    }
    return raccSceneFreeBase(ctx, scene);
}

}  // extern "C"
