// gen_pack_emu — k_gen_pack's decode (gen_pack_kernels.h) run on the HOST over every (work item, lane) and compared, word for word and
// segment by segment, with the host pack (cid_set_weight x 24) of the same seeded values; also checks that every 16-byte quad of the
// blob is produced exactly once.  Needs no GPU: it checks the index formulas, not the device's arithmetic (the GPU test
// tests/test_generator_pack_device.py does that).  Exit status 0 = identical.
//
//     make -C celebrity_image_denoiser_amd/csrc tools/gen_pack_emu && celebrity_image_denoiser_amd/csrc/tools/gen_pack_emu
#include "../cid_api.hip"

#include <random>

int main() {
    cid_handle_t h;
    if (cid_create(&h) != CID_OK) return 1;
    std::mt19937 rng(7);
    std::vector<std::vector<float>> P(CID_NUM_PARAMS);
    const float* ptr[CID_NUM_PARAMS];
    const float edge[] = {0.0f, -0.0f, 1.0f, -1.0f, 9.5367431640625e-07f, -9.5367431640625e-07f, 1e-6f, 3.0e4f, 0.3330078125f};
    for (int i = 0; i < CID_NUM_PARAMS; ++i) {
        const LayerDef& L = kLayers[i / 2];
        const bool bias = i & 1;
        const size_t n = bias ? L.cout : ref_weight_count(L);
        P[i].resize(n);
        std::normal_distribution<float> d(0.f, 0.05f);
        for (auto& v : P[i]) v = d(rng);
        for (size_t k = 0; k < 200 && k < n; ++k) P[i][rng() % n] = edge[rng() % 9];
        P[i][0] = -0.0f;
        P[i][n - 1] = 3.0e4f;
        int64_t shape[4];
        int nd = 4;
        if (bias) { shape[0] = L.cout; nd = 1; }
        else if (L.kind == CONVT) { shape[0] = L.cin; shape[1] = L.cout; shape[2] = 2; shape[3] = 2; }
        else { shape[0] = L.cout; shape[1] = L.cin; shape[2] = 3; shape[3] = 3; }
        if (cid_set_weight(h, cid_param_key(i), P[i].data(), shape, nd) != CID_OK) { printf("cid_set_weight: %s\n", cid_last_error(h)); return 1; }
        ptr[i] = P[i].data();
    }
    std::vector<unsigned> out(kBlob.total, 0xA5A5A5A5u);
    std::vector<unsigned char> hit(kBlob.total / 4, 0);
    const GenPackArgs a = gen_pack_args(ptr, out.data());
    printf("segments %d, work items %u, quads %zu\n", a.nseg, a.nitems, hit.size());
    size_t twice = 0;
    for (unsigned t = 0; t < a.nitems; ++t)
        for (int lane = 0; lane < 64; ++lane)
            gen_pack_item(a, t, lane, [&](unsigned q, const unsigned (&v)[4]) {
                if (q >= hit.size() || hit[q]++) { ++twice; return; }
                memcpy(&out[4 * (size_t)q], v, 16);
            });
    size_t never = 0;
    for (unsigned char c : hit) never += !c;
    printf("quads produced twice or out of range %zu, never %zu\n", twice, never);
    const unsigned* ref = reinterpret_cast<const unsigned*>(h->staging.data());
    size_t bad = 0;
    for (int i = 0;; ++i) {
        const char* name;
        size_t off, bytes;
        if (cid_packed_segment(i, &name, &off, &bytes) != CID_OK) break;
        size_t d = 0;
        for (size_t k = off / 4; k < (off + bytes) / 4; ++k) d += out[k] != ref[k];
        if (d) printf("%-22s offset %10zu bytes %9zu  differing words %zu\n", name, off, bytes, d);
        bad += d;
    }
    printf("differing words %zu of %zu\n", bad, (size_t)kBlob.total);
    cid_destroy(h);
    return (bad || twice || never) ? 1 : 0;
}
