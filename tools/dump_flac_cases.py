"""Write the FLAC streams the tests share (tests/flac_writer.py: the matrix, the planted streams, the rejection inputs) and
tests/golden/jfk_head.flac into a directory, for tools/fuzz_flac_frames.c:  python tools/dump_flac_cases.py DIR"""
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flac_writer as fw  # noqa: E402

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
cases = {name: data for name, data, *_ in fw.matrix()}
cases.update({f"planted{n}": fw.planted(n)[0] for n in (1, 40)})
cases.update({f"reject_{k}": v for k, v in fw.rejections()[0].items()})
for name, data in cases.items():
    with open(os.path.join(out, name + ".flac"), "wb") as f:
        f.write(data)
shutil.copy(os.path.join(ROOT, "tests", "golden", "jfk_head.flac"), os.path.join(out, "jfk_head.flac"))
print(f"{len(cases) + 1} files in {out}")
