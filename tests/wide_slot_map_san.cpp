// Stand-alone driver of kg_batch_slot_map (kg_host.cpp) for an AddressSanitizer + UndefinedBehaviorSanitizer build
// (tests/test_wide_batch_cpu.py compiles it with the host sources and runs it): random pod batches of every width
// class (2 / 4 / 8 slots, more than 8 resources), exact-size heap buffers so that any access past a batch, the 8 slot
// ids or the n spill bytes is reported, and the rule's invariants checked on every result.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "koord_gpu.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}

static int fail(const char *what, int n, int width) {
    fprintf(stderr, "FAIL %s (n = %d, width class %d)\n", what, n, width);
    return 1;
}

int main() {
    kg_config cfg;
    kg_config_default(&cfg);
    for (int r = 0; r < KG_NUM_RES; r++) cfg.fit_resource_weight[r] = r < 9 ? 1 : 0;
    const int sizes[] = {0, 1, 3, 64, 1000};
    int checked = 0;
    for (int width = 0; width < 4; width++) {       // resources the pods may request: 2, 4, 8, all 12
        const int nres = width == 0 ? 2 : width == 1 ? 5 : width == 2 ? 8 : KG_NUM_RES;
        for (int n : sizes) {
            std::vector<kg_pod_row> pods((size_t)n);
            if (n) memset(pods.data(), 0, sizeof(kg_pod_row) * (size_t)n);
            for (auto &p : pods) {
                p.flags = KG_POD_HAS_REQUEST | KG_POD_VALID;
                for (int r = 0; r < nres; r++) {
                    if (width == 1 && r == KG_RES_EPHEMERAL_STORAGE) continue;
                    if (rnd() % 3 == 0) continue;
                    p.request[r] = rnd() % 4;   // a present key with a zero request now and then
                    p.fit_score_request[r] = p.request[r];
                    p.request_present |= 1u << r;
                }
            }
            if (width == 0 || width == 1) cfg.fit_resource_weight[KG_RES_EPHEMERAL_STORAGE] = 0;
            else cfg.fit_resource_weight[KG_RES_EPHEMERAL_STORAGE] = 1;
            for (int r = 3; r < 9; r++) cfg.fit_resource_weight[r] = width >= 2 ? 1 : 0;
            int32_t n_slots = -7;
            std::vector<int32_t> slot_res(8, -7);
            std::vector<uint8_t> spill((size_t)n, 0xAB);
            for (int with_spill = 0; with_spill < 2; with_spill++) {
                const kg_status st = kg_batch_slot_map(&cfg, n ? pods.data() : nullptr, n, &n_slots, slot_res.data(),
                                                       with_spill && n ? spill.data() : nullptr);
                if (st != KG_OK) return fail("status", n, width);
                if (n_slots != 2 && n_slots != 4 && n_slots != 8) return fail("n_slots", n, width);
                if (slot_res[0] != KG_RES_CPU || slot_res[1] != KG_RES_MEMORY) return fail("cpu / memory", n, width);
                uint32_t held = 0;
                for (int s = 0; s < 8; s++) {
                    if (slot_res[s] < -1 || slot_res[s] >= KG_NUM_RES) return fail("slot id", n, width);
                    if (s >= n_slots && slot_res[s] != -1) return fail("unused slot", n, width);
                    if (slot_res[s] >= 0) {
                        if (held & (1u << slot_res[s])) return fail("repeated slot", n, width);
                        held |= 1u << slot_res[s];
                    }
                    if (n_slots == 8 && s > 2 && slot_res[s] >= 0 && slot_res[s] <= slot_res[s - 1])
                        return fail("ascending ids", n, width);
                }
                if (width < 2 && n_slots != (width == 0 ? 2 : n ? 4 : 2) && n > 3) return fail("legacy map", n, width);
                if (with_spill)
                    for (int i = 0; i < n; i++) {
                        if (spill[(size_t)i] > 1) return fail("spill byte", n, width);
                        // a pod compares every key it carries: outside the map ⇒ spill pod
                        const bool outside = (pods[(size_t)i].request_present & KG_SCALAR_RES_MASK & ~held) != 0;
                        if (outside && !spill[(size_t)i]) return fail("pod outside the map not marked", n, width);
                        if (spill[(size_t)i] && width < 3) return fail("spill pod in a batch of at most 8", n, width);
                    }
                checked++;
            }
        }
    }
    if (kg_batch_slot_map(nullptr, nullptr, 0, nullptr, nullptr, nullptr) == KG_OK) return fail("null arguments", 0, 0);
    printf("OK %d maps\n", checked);
    return 0;
}
