#!/usr/bin/env python3
"""Dump the engine's launch plans as canonical JSON, to compare two builds of the dispatch code byte for byte.

Host only (clasfv_max_clips and clasfv_forward_plan touch no device). For both compute dtypes, over the
no-variant set and every single bit of _lib.VARIANTS, and for each shape of SHAPES: max_clips and the full
forward plan (launches with every field and range, and the arena buffers). With no variants also the
sub-batched call of max_clips + 3 product clips. The dump is one JSON document with sorted keys; its SHA-256
goes to stderr, so two trees agree exactly when their hashes do.

    python tools/plan_dump.py > plans.json        # hash on stderr
    python tools/plan_dump.py --hash-only         # hash on stdout, no dump
"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clasfv_amd import _lib  # noqa: E402
from clasfv_amd.model import forward_plan, variant_flags  # noqa: E402

SHAPES = [(1, 8, 16, 32), (2, 16, 64, 48), (3, 24, 80, 112), (1, 32, 112, 112), (12, 32, 112, 112),
          (30, 32, 112, 112), (1, 64, 224, 224)]
PRODUCT_CLIP = (32, 112, 112)


def dump():
    lib = _lib.load()
    out = []
    for dtype in ("fp32", "bf16"):
        for variants in [()] + [(v,) for v in _lib.VARIANTS]:
            def entry(n, thw):
                return {"dtype": dtype, "variants": list(variants), "shape": [n, *thw],
                        "max_clips": lib.clasfv_max_clips(*thw, _lib.DTYPES[dtype], variant_flags(variants)),
                        "plan": forward_plan(n, *thw, dtype=dtype, variants=variants)}
            for n, *thw in SHAPES:
                out.append(entry(n, thw))
            if not variants:
                out.append(entry(lib.clasfv_max_clips(*PRODUCT_CLIP, _lib.DTYPES[dtype], 0) + 3, PRODUCT_CLIP))
    return json.dumps(out, sort_keys=True, indent=0, separators=(",", ":")) + "\n"


def main():
    text = dump()
    digest = hashlib.sha256(text.encode()).hexdigest()
    if "--hash-only" in sys.argv[1:]:
        print(digest)
        return
    sys.stdout.write(text)
    print(f"sha256 {digest}", file=sys.stderr)


if __name__ == "__main__":
    main()
