"""What the CPU suites of the four companion libraries (test_recon.py, test_mapped.py, test_typed.py, test_requant.py) check in
common about their sources and their build: a companion's directory and rustyhgi_amd/companion/, which all four include."""
import os
import re

from conftest import ROOT

COMPANION_DIR = os.path.join(ROOT, "rustyhgi_amd", "companion")
COMPANION_FILES = ["companion.mk", "hgi_entry.h", "hgi_sides.h"]


def check_sources(directory, listing=None):
    """Stateless and switch-free sources: no environment read, no tuning switch, no device allocation, no ctx -- in every file
    of `directory` and of the shared layer; and exactly the files expected, where a listing is given."""
    for d, want in ((directory, listing), (COMPANION_DIR, COMPANION_FILES)):
        files = sorted(f for f in os.listdir(d) if os.path.isfile(os.path.join(d, f)))
        if want is not None:
            assert files == sorted(want), (d, files)
        for fn in files:
            src = open(os.path.join(d, fn)).read()
            assert "getenv" not in src and "KNOBS_ENV" not in src and "HGI_KNOB(" not in src, (d, fn)
            assert "hipMalloc" not in src and "hgi_ctx" not in src, (d, fn)      # no device allocation, no ctx
    # the shared headers name no switch either (the `strings` check of each library sees what they compile to)
    for fn in ("hgi_entry.h", "hgi_sides.h"):
        assert not re.search(r'"[^"\n]*HGI_[A-Z0-9_]+[^"\n]*"', open(os.path.join(COMPANION_DIR, fn)).read()), fn


def makefile(directory, name, fused):
    """The text make reads for a companion: its Makefile -- NAME, the direction's FUSED unit and the include, nothing else --
    followed by companion.mk with the two variables expanded."""
    mk = open(os.path.join(directory, "Makefile")).read()
    code = [l.strip() for l in mk.splitlines() if l.strip() and not l.startswith("#")]
    assert code == ["NAME := " + name, "FUSED := " + fused, "include ../companion/companion.mk"], code
    shared = open(os.path.join(COMPANION_DIR, "companion.mk")).read()
    assert len(re.findall(r"\$\(CSRC\)/hgi_fused_impl\.h", shared)) == 1, "the tile procedure's dependency list stands once"
    return mk + shared.replace("$(NAME)", name).replace("$(FUSED)", fused)
