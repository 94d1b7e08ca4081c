"""Every switch the engine and the front-end read from the environment is documented: each KMDB_* name passed to getenv under
kmer-db_amd/csrc and kmer-db_amd/host appears in README.md."""
import os
import re

from conftest import ROOT


def _sources():
    for sub in ("csrc", "host"):
        top = os.path.join(ROOT, "kmer-db_amd", sub)
        for dirpath, _, names in os.walk(top):
            for name in sorted(names):
                if name.endswith((".hip", ".cpp", ".h", ".hpp")):
                    yield os.path.join(dirpath, name)


def test_every_switch_read_from_the_environment_is_in_the_readme():
    # a name given to getenv directly, or to any helper whose argument ends up there: every "KMDB_..." string literal passed to a call
    literal = re.compile(r'\w+\(\s*"(KMDB_[A-Z0-9_]+)"\s*\)')
    read = {}
    for path in _sources():
        with open(path, encoding="utf-8") as f:
            text = f.read()
        for name in literal.findall(text):
            read.setdefault(name, os.path.relpath(path, ROOT))
    assert len(read) >= 30, sorted(read)                         # (the patterns still find the reads)
    with open(os.path.join(ROOT, "README.md"), encoding="utf-8") as f:
        readme = f.read()
    documented = set(re.findall(r"KMDB_[A-Z0-9_]+", readme))
    missing = {name: where for name, where in read.items() if name not in documented}
    assert not missing, "switches read but not in README.md: %s" % sorted(missing.items())
