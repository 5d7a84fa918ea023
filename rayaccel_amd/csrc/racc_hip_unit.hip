// racc_hip.hip's scene upload / free are compiled under other names (not exported: racc_hip.map) and wrapped by racc_refit.inc, which keeps
// what a refit needs of the uploaded blob beside the scene handle; racc_hip.hip itself is unchanged.  racc_refit.inc's wrappers are in
// turn compiled under other names and wrapped by racc_world.inc, which notes the context a scene was uploaded on (instancing refuses
// another context's scene): the public racc_hip_scene_upload / racc_hip_scene_free are the ones at the end of that file.
#define racc_hip_scene_upload raccSceneUploadBase
#define racc_hip_scene_free raccSceneFreeBase
#include "racc_hip.hip"
#undef racc_hip_scene_upload
#undef racc_hip_scene_free
#include "racc_occlusion.inc"
#define racc_hip_scene_upload raccSceneUploadRefit
#define racc_hip_scene_free raccSceneFreeRefit
#include "racc_refit.inc"
#undef racc_hip_scene_upload
#undef racc_hip_scene_free
#include <array>
#include "racc_world.inc"
