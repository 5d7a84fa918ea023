#include "racc_hip.hip"
#include "racc_occlusion.inc"
