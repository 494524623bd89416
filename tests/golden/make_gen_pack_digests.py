"""Records the SHA-256 of every segment (names and ranges from cid_packed_segment) and of the whole blob of pack_weights_host() for
the three weight sets of tests/test_generator_pack_device.py, as tests/golden/gen_pack_digests.json.

RUN THIS ONLY AT A COMMIT THAT STILL HAS THE SCATTER PACK: cd1dc5e ("Add a device-side bicubic resize that matches Pillow bit for
bit"), the last one whose cid_set_weight writes the blob with packed_index*, pack_winograd_u and pack_winograd42_u, a second
statement of the layout written independently of gen_pack_kernels.h.  Since then the host pack runs the gather code of
gen_pack_kernels.h, so the recorded digests are the only independent statement of the layout left.  Regenerating the file from the
code under test is circular: it would record whatever that code produces, a wrong layout included.  A layout that changes on purpose
needs digests from an implementation written apart from the one under test.

    git checkout cd1dc5e -- celebrity_image_denoiser_amd/csrc && python __graft_entry__.py && python tests/golden/make_gen_pack_digests.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

RECORDED_AT = "cd1dc5e"


def main():
    import test_generator_pack_device as t

    segs, _ = t.segments()
    sets = {}
    for kind in t.WSETS:
        blob = t.host_blob(kind).numpy().tobytes()
        sets[kind] = {"blob": hashlib.sha256(blob).hexdigest(),
                      "segments": {name: hashlib.sha256(blob[off:off + size]).hexdigest() for name, off, size in segs}}
    doc = {"recorded_at": RECORDED_AT, "bytes": len(blob), "ranges": {name: f"{off}+{size}" for name, off, size in segs}, "sets": sets}
    path = os.path.join(HERE, "gen_pack_digests.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)   # one short line per segment and weight set
        f.write("\n")
    print(f"{os.path.basename(path)}: {len(segs)} segments x {len(sets)} weight sets, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
