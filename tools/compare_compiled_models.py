#!/usr/bin/env python3
"""Show that a change to the model compiler left its output alone: compile every configuration with two trees, compare byte for byte.

    git worktree add /tmp/parent <parent commit>          (or any other checkout of the commit to compare against)
    python tools/compare_compiled_models.py /tmp/parent

In one child process per tree (the parent checkout and the tree this file is in), for each of the entries of CONFIGS and
TEST_CONFIGS: `compile_model(**kw, ref_root=tests/golden/hsr_data).to_bytes()` and the files `emit_mjcf` writes.  Both trees
read the data files of THIS tree.  The blobs must be identical for every configuration.  Every MJCF file must be identical for
the configurations both trees can emit; a configuration only this tree can emit (the parent's emit_mjcf had no `block_geom`)
must parse, and its injected block0 geom must carry what `block_geom` asks for (a mesh geom has no `size`).  Exit status 1 if
anything differs."""
import hashlib
import subprocess
import sys
import tempfile
import xml.etree.ElementTree as ET
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
REF_DATA = HERE / "tests" / "golden" / "hsr_data"


def dump(tree, out):
    """Child process: write <out>/<cfg>.hsrm and <out>/mjcf/<cfg>*.xml with the compiler of `tree`."""
    sys.path.insert(0, str(tree))
    from hsr_env_amd import compiler as hc
    assert Path(hc.__file__).resolve().is_relative_to(Path(tree).resolve()), hc.__file__
    for name, kw in dict(hc.CONFIGS, **hc.TEST_CONFIGS).items():
        (out / f"{name}.hsrm").write_bytes(hc.compile_model(**kw, ref_root=REF_DATA).to_bytes())
        xml_kw = {k: v for k, v in kw.items() if k != "plane_convex_points"}      # not an XML property
        try:
            hc.emit_mjcf(out / "mjcf", name, **xml_kw, ref_root=REF_DATA)
        except TypeError as e:
            print(f"{tree}: cannot emit {name}: {e}")


def check_block_geom(hc_configs, name, files):
    """A configuration the parent could not emit: parses, and block0's geom is what block_geom describes."""
    bad = []
    want = hc_configs[name].get("block_geom") or {}
    for f in files:
        root = ET.parse(f).getroot()
        for g in root.findall("worldbody/body[@name='block0']/geom"):
            if any(g.get(k) != v for k, v in want.items()) or (want.get("type") == "mesh" and g.get("size") is not None):
                bad.append(f"{f.name}: block0 geom {g.attrib} does not carry {want}")
    if not any(ET.parse(f).getroot().find("worldbody/body[@name='block0']/geom") is not None for f in files):
        bad.append(f"{name}: no file holds the injected block0 geom")
    return bad


def main(parent):
    with tempfile.TemporaryDirectory() as tmp:
        outs = {}
        for tag, tree in (("parent", Path(parent).resolve()), ("branch", HERE)):
            outs[tag] = Path(tmp) / tag
            (outs[tag] / "mjcf").mkdir(parents=True)
            subprocess.run([sys.executable, __file__, "--dump", str(tree), str(outs[tag])], check=True, cwd=tmp)
        sys.path.insert(0, str(HERE))
        from hsr_env_amd import compiler as hc
        configs = dict(hc.CONFIGS, **hc.TEST_CONFIGS)
        bad, nxml = [], 0
        seen = {t: sorted(f.stem for f in outs[t].glob("*.hsrm")) for t in outs}
        if not (seen["parent"] == seen["branch"] == sorted(configs)):
            print(f"the trees compiled different configurations: {seen}")
            return 1
        for name in configs:
            a, b = ((outs[t] / f"{name}.hsrm").read_bytes() for t in ("parent", "branch"))
            print(f"{name:12s} blob {len(b):7d} B  sha256 {hashlib.sha256(b).hexdigest()[:16]}  {'same' if a == b else 'DIFFERS'}")
            if a != b:
                bad.append(f"{name}: blobs differ")
            fa, fb = (sorted((outs[t] / "mjcf").glob(f"{name}.xml")) + sorted((outs[t] / "mjcf").glob(f"{name}__*"))
                      for t in ("parent", "branch"))
            if not fb:
                bad.append(f"{name}: this tree cannot emit it")
            elif not fa:
                bad += check_block_geom(configs, name, fb)
                print(f"{name:12s} mjcf  {len(fb)} files, only this tree emits them: parsed, block0 geom checked")
            else:
                if [f.name for f in fa] != [f.name for f in fb]:
                    bad.append(f"{name}: different MJCF files")
                bad += [f"{x.name}: MJCF differs" for x, y in zip(fa, fb) if x.read_bytes() != y.read_bytes()]
                nxml += len(fb)
        if not configs or not nxml:
            bad.append(f"nothing to compare: {len(configs)} configurations, {nxml} MJCF files both trees emit")
        print("\n".join(bad) if bad else "", end="\n" if bad else "")
        print(f"{len(configs)} blobs and {nxml} MJCF files compared: {len(bad)} differing")
        return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--dump":
        sys.exit(dump(Path(sys.argv[2]), Path(sys.argv[3])))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
