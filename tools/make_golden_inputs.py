"""Stores the reference's input files that tests/test_msh_io.py and tests/test_scene_script.py read, as fixtures under tests/golden/:
  tests/golden/ref_meshes/<name>.msh.gz    five tet meshes of input/tetMeshes (gzip of the file as shipped)
  tests/golden/ref_scene_files.tar.gz      every scene script (*.txt) under input/, paths relative to input/

    python tools/make_golden_inputs.py REFERENCE_ROOT"""
import gzip
import io
import os
import sys
import tarfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MESHES = ("bar-2523", "mat20x20", "cube", "sphere1K", "mat40x40")


def main(ref_root):
    inp = os.path.join(ref_root, "input")
    os.makedirs(os.path.join(GOLDEN, "ref_meshes"), exist_ok=True)
    for name in MESHES:
        data = open(os.path.join(inp, "tetMeshes", name + ".msh"), "rb").read()
        with open(os.path.join(GOLDEN, "ref_meshes", name + ".msh.gz"), "wb") as f:
            f.write(gzip.compress(data, compresslevel=9, mtime=0))
    scripts = []
    for root, _, files in os.walk(inp):
        scripts += [os.path.relpath(os.path.join(root, f), inp) for f in files if f.endswith(".txt")]
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.USTAR_FORMAT) as tar:
        for rel in sorted(scripts):
            data = open(os.path.join(inp, rel), "rb").read()
            info = tarfile.TarInfo(rel)
            info.size, info.mode = len(data), 0o644
            tar.addfile(info, io.BytesIO(data))
    with open(os.path.join(GOLDEN, "ref_scene_files.tar.gz"), "wb") as f:
        f.write(gzip.compress(buf.getvalue(), compresslevel=9, mtime=0))
    print(f"{len(MESHES)} meshes, {len(scripts)} scene scripts")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
