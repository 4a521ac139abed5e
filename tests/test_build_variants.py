"""The variant tables of gaussianrpg_amd/build.py against the sources: every -DNAME[=...] flag of an
entry must name something the unit it recompiles (or common.h) actually reads.  A flag that nothing
reads builds a copy of the default library under another name."""
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
