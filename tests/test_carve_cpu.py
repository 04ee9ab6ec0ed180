"""The layout half of the host-kind staging (csrc/mcs_carve.h) on its own, without a GPU: every piece 256-byte aligned and at least as long as asked,
pieces disjoint and in the order of declaration, a zero-byte piece legal with a slot of its own, the block's size the sum of the slots; and the binding layout
next to it (Layout), whose offsets and total are Carve's."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_carve_layout(tmp_path):
    exe = tmp_path / "carve_driver"
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "multicol-slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "carve_driver.cpp"), "-o", str(exe)])
    sizes = [0, 1, 255, 256, 257, 0, 0, 4096, 3, 1 << 33, 0]
    lines = subprocess.check_output([str(exe)] + [str(s) for s in sizes]).decode().split("\n")
    pieces = [tuple(int(v) for v in ln.split()) for ln in lines[:len(sizes)]]
    total = int(lines[len(sizes)])
    end = 0
    for want, (off, size) in zip(sizes, pieces):
        assert off % 256 == 0 and size % 256 == 0
        assert off == end                       # declaration order, no gap, no overlap
        assert size >= max(want, 1) and size - max(want, 1) < 256   # nothing but the alignment
        end = off + size
    assert total == end == sum(size for _, size in pieces)
    assert len({off for off, _ in pieces}) == len(pieces)           # zero-byte pieces have addresses of their own
    # the binding layout (Layout::piece / place): every bound pointer reads base + the offset Carve::take gives, in declaration order; a piece without a
    # pointer takes its room (100 bytes -> one 256-byte slot behind the rest)
    rest = lines[len(sizes) + 1:]
    bound = [int(v) for v in rest[:len(sizes)]]
    assert bound == [off for off, _ in pieces]
    assert int(rest[len(sizes)]) == total + 256
