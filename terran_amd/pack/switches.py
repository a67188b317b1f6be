"""What decides a packed program besides the weights and the precision: the environment switches the packers read, and the
packer's own sources."""
import os

# every environment switch a packer reads: a program packed with one of them set must never be served to a default run
# (runtime.packed_program bypasses the on-disk repack cache then, and keys its in-process memo on them)
PACK_SWITCHES = ('TERRAN_AMD_NO_FUSED_FRONT', 'TERRAN_AMD_NO_DETECTOR_LANES', 'TERRAN_AMD_NO_ACT_SCALES')


def active_switches():
    return tuple((k, os.environ[k]) for k in PACK_SWITCHES if os.environ.get(k))


_SOURCE_TAG = []


def source_tag():
    """Short hash of the packer's own sources: a repack cache written by another version of this package / arch.py is not read.
    Computed once per process; an install without the .py files (pyc-only, zip) has nothing to hash: it returns None and
    runtime.packed_program then runs WITHOUT the on-disk cache (two such installs of different packers would share one key)."""
    if not _SOURCE_TAG:
        import hashlib
        h = hashlib.sha256()
        here = os.path.dirname(os.path.abspath(__file__))
        try:
            for f in sorted(f for f in os.listdir(here) if f.endswith('.py')) + [os.path.join(os.pardir, 'arch.py')]:
                with open(os.path.join(here, f), 'rb') as fh:
                    h.update(fh.read())
            _SOURCE_TAG.append(h.hexdigest()[:10])
        except OSError:
            _SOURCE_TAG.append(None)
    return _SOURCE_TAG[0]
