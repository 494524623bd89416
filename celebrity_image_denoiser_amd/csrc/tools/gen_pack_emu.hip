// gen_pack_emu — the stand-alone host check of the generator's pack (gen_pack_kernels.h), which the host (cid_set_weight) and the device
// (k_gen_pack) both compile.  Needs no GPU.  It checks what is not the layout itself (tests/golden/gen_pack_digests.json pins that):
//   (a) over all work items of the blob, every 16-byte quad is produced exactly once;
//   (b) the blob that cid_set_weight stages tensor by tensor, in cid_param_key order and in reverse order, equals that whole-blob gather;
//   (c) setting one tensor again with other values changes every segment it feeds and no byte of any other segment or table.
// Every emit of the host pack is a store at a computed index: build with -fsanitize=address,undefined (EXTRA=...) to have them checked.
// Exit status 0 = all three hold.
//
//     make -C celebrity_image_denoiser_amd/csrc tools/gen_pack_emu && celebrity_image_denoiser_amd/csrc/tools/gen_pack_emu
#include "../cid_api.hip"

#include <chrono>
#include <random>

static int set_param(cid_handle_t h, int i, const std::vector<float>& v) {
    const LayerDef& L = kLayers[i / 2];
    int64_t shape[4] = {L.cout, L.cin, 3, 3};
    if (L.kind == CONVT && !(i & 1)) { shape[0] = L.cin; shape[1] = L.cout; shape[2] = shape[3] = 2; }
    const int rc = cid_set_weight(h, cid_param_key(i), v.data(), shape, (i & 1) ? 1 : 4);
    if (rc != CID_OK) printf("cid_set_weight: %s\n", cid_last_error(h));
    return rc;
}

int main() {
    cid_handle_t fwd, rev;
    if (cid_create(&fwd) != CID_OK || cid_create(&rev) != CID_OK) return 1;
    std::mt19937 rng(7);
    std::vector<std::vector<float>> P(CID_NUM_PARAMS);
    const float* ptr[CID_NUM_PARAMS];
    const float edge[] = {0.0f, -0.0f, 1.0f, -1.0f, 9.5367431640625e-07f, -9.5367431640625e-07f, 1e-6f, 3.0e4f, 0.3330078125f};
    for (int i = 0; i < CID_NUM_PARAMS; ++i) {
        const LayerDef& L = kLayers[i / 2];
        const size_t n = (i & 1) ? L.cout : ref_weight_count(L);
        P[i].resize(n);
        std::normal_distribution<float> d(0.f, 0.05f);
        for (auto& v : P[i]) v = d(rng);
        for (size_t k = 0; k < 200 && k < n; ++k) P[i][rng() % n] = edge[rng() % 9];
        P[i][0] = -0.0f;
        P[i][n - 1] = 3.0e4f;
        ptr[i] = P[i].data();
    }

    // (a)
    std::vector<unsigned> out(kBlob.total, 0xA5A5A5A5u);
    std::vector<unsigned char> hit(kBlob.total / 4, 0);
    const GenPackArgs a = gen_pack_args(ptr, out.data());
    printf("segments %d, work items %u, quads %zu\n", a.nseg, a.nitems, hit.size());
    size_t twice = 0, never = 0;
    for (unsigned t = 0; t < a.nitems; ++t)
        for (int lane = 0; lane < 64; ++lane)
            gen_pack_item(a, t, lane, [&](unsigned q, const unsigned (&v)[4]) {
                if (q >= hit.size() || hit[q]++) { ++twice; return; }
                memcpy(&out[4 * (size_t)q], v, 16);
            });
    for (unsigned char c : hit) never += !c;
    printf("(a) quads produced twice or out of range %zu, never %zu\n", twice, never);

    // (b)
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < CID_NUM_PARAMS; ++i)
        if (set_param(fwd, i, P[i]) != CID_OK) return 1;
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int i = CID_NUM_PARAMS - 1; i >= 0; --i)
        if (set_param(rev, i, P[i]) != CID_OK) return 1;
    const size_t bytes = kBlob.total * sizeof(float);
    const bool same_f = !memcmp(fwd->staging.data(), out.data(), bytes), same_r = !memcmp(rev->staging.data(), out.data(), bytes);
    printf("(b) staged in key order %s, in reverse order %s the whole-blob gather (24 x cid_set_weight: %.3f s)\n", same_f ? "equals" : "DIFFERS FROM",
           same_r ? "equals" : "DIFFERS FROM", secs);

    // (c)
    size_t wrong = 0;
    std::vector<float> before(fwd->staging);
    for (int i = 0; i < CID_NUM_PARAMS; ++i) {
        for (auto& v : P[i]) v = v * 1.5f + 0.25f;
        if (set_param(fwd, i, P[i]) != CID_OK) return 1;
        for (int k = 0; k < a.nseg; ++k) {
            const size_t off = 4 * (size_t)a.seg[k].q0, n = 4 * (size_t)a.seg[k].nq;
            const bool changed = memcmp(&before[off], &fwd->staging[off], n * sizeof(float)) != 0;
            const bool fed = a.seg[k].fam != GP_TAB && a.seg[k].src == i;
            if (changed != fed) { ++wrong; printf("    %s: segment %s %s\n", cid_param_key(i), blob_segments()[k].name.c_str(), changed ? "changed" : "did not change"); }
        }
        before = fwd->staging;
    }
    printf("(c) segments that changed without being fed, or were fed and did not change: %zu\n", wrong);
    cid_destroy(fwd);
    cid_destroy(rev);
    return (twice || never || !same_f || !same_r || wrong) ? 1 : 0;
}
