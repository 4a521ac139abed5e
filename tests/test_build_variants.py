"""The variant tables of gaussianrpg_amd/build.py against the sources: every -DNAME[=...] flag of an
entry must name something the unit it recompiles (or common.h) actually reads.  A flag that nothing
reads builds a copy of the default library under another name.  And the sources against the build: every quoted
include exists and makes the objects stale, every unit is built."""
import glob
import os
import re

from gaussianrpg_amd import build


def _read(name):
    with open(os.path.join(build.CSRC, name)) as f:
        return f.read()


def test_every_variant_flag_is_read_by_its_unit():
    assert not set(build.VARIANTS) & set(build.EXPERIMENT_VARIANTS)
    common = _read("common.h")
    checked = 0
    for table in (build.VARIANTS, build.EXPERIMENT_VARIANTS):
        for name, spec in table.items():
            assert spec, name
            for unit, flags in spec.items():
                assert unit in build.HIP_UNITS, (name, unit)
                source = _read(unit)
                for flag in flags:
                    m = re.fullmatch(r"-D([A-Za-z_][A-Za-z0-9_]*)(=.*)?", flag)
                    assert m, "%s: %r is not a -DNAME[=value] flag" % (name, flag)
                    word = re.compile(r"\b%s\b" % re.escape(m.group(1)))
                    assert word.search(source) or word.search(common), \
                        "%s: %s is read neither by %s nor by common.h" % (name, m.group(1), unit)
                    checked += 1
    assert checked >= len(build.VARIANTS) + len(build.EXPERIMENT_VARIANTS)


def test_every_include_exists_and_every_unit_and_header_is_known_to_the_build():
    sources = glob.glob(os.path.join(build.CSRC, "*.hip")) + glob.glob(os.path.join(build.CSRC, "*.h")) + \
        [os.path.join(build.CSRC, "torch_binding.cpp")]
    stale = {os.path.realpath(h) for h in build.headers()}
    seen = 0
    for src in sources:
        with open(src) as f:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M):
                path = os.path.realpath(os.path.join(os.path.dirname(src), inc))
                assert os.path.isfile(path), "%s includes %s, which does not exist" % (os.path.basename(src), inc)
                if os.path.dirname(path) == os.path.realpath(build.CSRC):
                    assert path in stale, "%s: an edit to %s would rebuild nothing" % (os.path.basename(src), inc)
                seen += 1
    assert seen >= len(build.HIP_UNITS)     # every unit includes at least common.h
    units = {os.path.basename(p) for p in glob.glob(os.path.join(build.CSRC, "*.hip"))}
    assert units == set(build.HIP_UNITS)
