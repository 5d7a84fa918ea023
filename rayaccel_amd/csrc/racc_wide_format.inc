// racc_wide_format.inc — racc_host_scene_wide_nodes: the 4-wide device records of a node blob without a GPU (for tools and tests), by the very
// collapseWide / quantiseWide of racc_scene_format.inc that racc_hip_scene_upload runs, with the same refusals.  Textually included by
// racc_hip_unit.hip behind racc_hip.hip (not a hashed file: DESIGN.md §3, the fingerprint rule).
extern "C" {

int racc_host_scene_wide_nodes(const void* nodes64, uint32_t node_count, uint32_t pair_count, uint32_t remap_count, int format,
                               void* out, uint32_t capacity, uint32_t* count, uint32_t* stack_bound) {
    if (!nodes64 || !count || !stack_bound) return fail(RACC_HIP_ERR_INVALID, "wide_nodes: NULL argument");
    *count = 0; *stack_bound = 0;
    if (format != 45 && format != 50) return fail(RACC_HIP_ERR_INVALID, "wide_nodes: format must be 45 (128 B records) or 50 (64 B compressed records)");
    racc_hip_scene_info info{};
    if (int rc = validateScene(static_cast<const GpuNodeHost*>(nodes64), node_count, pair_count, remap_count, info)) return rc;
    std::vector<WideNode> wide;
    uint32_t bound = 0;
    collapseWide(static_cast<const GpuNodeHost*>(nodes64), node_count, wide, bound);
    std::vector<WideNodeQ> packed;
    if (format == 50) if (int rc = quantiseWide(wide, packed)) return rc;
    *count = uint32_t(wide.size()); *stack_bound = bound;
    if (out) {
        if (capacity < wide.size()) return fail(RACC_HIP_ERR_INVALID, "wide_nodes: capacity too small");
        if (format == 50) std::memcpy(out, packed.data(), packed.size() * sizeof(WideNodeQ));
        else std::memcpy(out, wide.data(), wide.size() * sizeof(WideNode));
    }
    return RACC_HIP_OK;
}

}  // extern "C"
