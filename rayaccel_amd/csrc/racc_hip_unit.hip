// racc_hip.hip's scene upload / free are compiled under other names (not exported: racc_hip.map) and wrapped by racc_refit.inc, which keeps
// what a refit needs of the uploaded blob beside the scene handle; racc_hip.hip itself is unchanged.
#define racc_hip_scene_upload raccSceneUploadBase
#define racc_hip_scene_free raccSceneFreeBase
#include "racc_hip.hip"
#undef racc_hip_scene_upload
#undef racc_hip_scene_free
#include "racc_occlusion.inc"
#include "racc_refit.inc"
