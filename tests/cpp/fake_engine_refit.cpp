// fake_engine_refit — the refit entries of the C-ABI for the GPU-free stand-in engine (fake_engine.cpp, `make tsan`): racc_api.cpp's
// racc::updateScene refers to them, the ThreadSanitizer driver never calls it.  TEST INFRASTRUCTURE: they refit nothing.
#include "racc_hip.h"

struct racc_hip_refit { int unused; };

extern "C" {
int racc_hip_refit_create(racc_hip_ctx*, racc_hip_scene*, const uint32_t*, uint32_t, uint32_t, racc_hip_refit** out) { *out = new racc_hip_refit{0}; return RACC_HIP_OK; }
int racc_hip_refit_destroy(racc_hip_ctx*, racc_hip_refit* r) { delete r; return RACC_HIP_OK; }
int racc_hip_scene_refit(racc_hip_ctx*, racc_hip_refit*, const float*, uint32_t) { return RACC_HIP_OK; }
}
