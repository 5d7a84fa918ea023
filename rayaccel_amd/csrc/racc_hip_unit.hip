// One translation unit: racc_hip.hip, unchanged, with the later features behind it.  racc_hip.hip's scene upload / free are compiled under
// internal names (not exported: racc_hip.map); the public racc_hip_scene_upload / racc_hip_scene_free are racc_scene_registry.inc's, which
// wrap them once and keep what refit and instancing need to know about a scene.  racc_query.inc holds what the query kernels share.
#define racc_hip_scene_upload raccSceneUploadBase
#define racc_hip_scene_free raccSceneFreeBase
#include "racc_hip.hip"
#undef racc_hip_scene_upload
#undef racc_hip_scene_free
#include "racc_scene_registry.inc"
#include "racc_query.inc"
#include "racc_occlusion.inc"
#include "racc_refit.inc"
#include "racc_refit_wide.inc"
#include <array>
#include "racc_world.inc"
#include "racc_world_occlusion.inc"
#include "racc_world_rule.h"
#include "racc_world_refit.inc"
#include "racc_world_rebuild_rule.h"
#include "racc_world_rebuild.inc"
#include "racc_scene_rebuild_rule.h"
#include "racc_scene_rebuild.inc"
#include "racc_wide_format.inc"
