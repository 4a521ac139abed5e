"""Generate tests/golden/ref_letterbox.json.  Needs a checkout of the reference (GaussianRPG); never run by a test:

    python tests/golden/make_golden_letterbox.py <path to the reference>

Cuts ``letterbox`` out of the reference's utils/augmentations.py with ``ast`` (the module itself imports cv2 and
torchvision, which are not installed here) and executes it with a stub in place of ``cv2`` whose ``resize`` and
``copyMakeBorder`` only record the size and the borders they are asked for.  The file holds numbers only: for every
case the source size and the options, and what letterbox derives from them -- the resized size (as cv2 takes it:
width, height; null when cv2.resize is not called), the borders, the output shape, ratio and (dw, dh).
"""
import ast
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class _Cv2Stub:
    INTER_LINEAR = 1
    BORDER_CONSTANT = 0

    def __init__(self):
        self.resized = None
        self.border = None

    def resize(self, im, size, interpolation=None):
        assert interpolation == self.INTER_LINEAR
        self.resized = [int(size[0]), int(size[1])]        # (width, height)
        return np.zeros((size[1], size[0], 3), np.uint8)

    def copyMakeBorder(self, im, top, bottom, left, right, kind, value=None):
        assert kind == self.BORDER_CONSTANT and tuple(value) == (114, 114, 114)
        self.border = [int(top), int(bottom), int(left), int(right)]
        return np.zeros((im.shape[0] + top + bottom, im.shape[1] + left + right, 3), np.uint8)


def _letterbox(stub, ref):
    path = os.path.join(ref, "utils", "augmentations.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "letterbox"]
    assert len(fn) == 1
    ns = {"np": np, "cv2": stub}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["letterbox"]


# (height, width, new_shape, options)
CASES = [
    # the reference's own configuration: imgsz = image width (simulator.py:144, object_detector.py:72)
    (1066, 1600, 1600, {}),
    (1280, 1920, 1920, {}),
    (1066, 1600, 1600, {"stride": 64}),
    (375, 1242, 1242, {}),
    # a smaller detector
    (1280, 1920, 640, {}),
    (1066, 1600, 640, {}),
    (375, 1242, 640, {}),
    (1280, 1920, 640, {"stride": 64}),
    (1066, 1600, 640, {"stride": 64}),
    (1280, 1920, 1280, {}),
    (1280, 1920, 960, {}),            # both scales exactly 1/2
    # tuple new_shape
    (1280, 1920, (384, 640), {}),
    (1280, 1920, (384, 640), {"auto": False}),
    (1280, 1920, (384, 640), {"auto": False, "scaleFill": True}),
    (1280, 1920, (384, 640), {"scaleFill": True}),          # auto wins over scaleFill
    (1066, 1600, (640, 480), {"auto": False, "scaleFill": True}),
    # every flag combination on a small upscaled source
    (48, 64, 640, {"auto": False, "scaleup": False}),
    (48, 64, 640, {"auto": True, "scaleup": False}),
    (48, 64, 640, {"auto": False, "scaleup": True}),
    (48, 64, 640, {"auto": True, "scaleup": True}),
    (48, 64, 640, {"auto": False, "scaleFill": True, "scaleup": False}),
    (48, 64, 640, {"auto": False, "scaleFill": True, "scaleup": True}),
    (48, 64, 640, {"auto": True, "scaleFill": True, "scaleup": False}),
    # the GPU tests' shapes
    (40, 64, 64, {}),
    (64, 64, 64, {}),
    (96, 160, 64, {}),
    (37, 53, 64, {}),
    (5, 7, 20, {}),
    (37, 53, 50, {"auto": False}),
    (37, 53, (40, 72), {"auto": False, "scaleFill": True}),
    # shape * r lands on a half: round() is round-half-to-even
    (5, 20, 10, {"auto": False}),       # 5 * 0.5 = 2.5 -> 2
    (7, 20, 10, {"auto": False}),       # 7 * 0.5 = 3.5 -> 4
    (20, 5, 10, {}),                    # the same along the width
    (50, 100, 25, {"stride": 64}),      # 50 * 0.25 = 12.5 -> 12
    (30, 100, 25, {"auto": False}),     # 30 * 0.25 = 7.5 -> 8
    # portrait
    (1920, 1280, 640, {}),
]


def main(ref):
    rows = []
    for H, W, new_shape, opt in CASES:
        stub = _Cv2Stub()
        letterbox = _letterbox(stub, ref)
        kw = dict(auto=True, scaleFill=False, scaleup=True, stride=32)
        kw.update(opt)
        im, ratio, dwdh = letterbox(np.zeros((H, W, 3), np.uint8), new_shape, **kw)
        rows.append({"height": H, "width": W, "new_shape": new_shape if isinstance(new_shape, int) else list(new_shape),
                     "auto": kw["auto"], "scaleFill": kw["scaleFill"], "scaleup": kw["scaleup"], "stride": kw["stride"],
                     "resized_wh": stub.resized, "border": stub.border, "out_shape": [int(im.shape[0]), int(im.shape[1])],
                     "ratio": [float(ratio[0]), float(ratio[1])], "dwdh": [float(dwdh[0]), float(dwdh[1])]})
    with open(os.path.join(HERE, "ref_letterbox.json"), "w") as f:
        json.dump({"source": "utils/augmentations.py:121-151 (letterbox), cv2 stubbed", "cases": rows}, f, indent=1)
        f.write("\n")
    print("wrote %d cases" % len(rows))


if __name__ == "__main__":
    main(sys.argv[1])
