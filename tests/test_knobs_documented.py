"""The library's environment knobs and docs/KNOBS.md say the same thing: every FBBEV_* name handed to the knob readers of
fb_bev_amd/csrc/capi_common.h is a row of the document's library table and the other way round, and nothing else in the C ABI's
sources touches the environment.  Source text only: no GPU, no library."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'fb_bev_amd', 'csrc')
READERS = ('fbbev_env_int', 'fbbev_env_str', 'FBBEV_KNOB_EMU_INT')


def sources():
    files = sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')))
    assert files
    return {os.path.basename(f): open(f).read() for f in files}


def strip_comments(text):
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return re.sub(r'//[^\n]*', '', text)


def knobs_read():
    names = set()
    for text in sources().values():
        names |= set(re.findall(r'\b(?:%s)\s*\(\s*"(FBBEV_\w+)"' % '|'.join(READERS), strip_comments(text)))
    return names


def knobs_documented():
    doc = open(os.path.join(ROOT, 'docs', 'KNOBS.md')).read()
    section = re.search(r'^## Library.*?(?=^## )', doc, flags=re.S | re.M).group(0)
    names = set()
    for row in re.findall(r'^\|(.*?)\|', section, flags=re.M):      # first column of the table
        names |= set(re.findall(r'`(FBBEV_\w+)`', row))
    return names


def test_every_knob_the_library_reads_is_documented_and_the_other_way_round():
    read, documented = knobs_read(), knobs_documented()
    # the scan sees every reader: an integer knob, a string knob, an emulator-only knob
    assert {'FBBEV_DA_FUSED', 'FBBEV_HISTORY_WARP', 'FBBEV_ROWS_LINEAR_RT'} <= read, sorted(read)
    assert read == documented, {'read, not in docs/KNOBS.md': sorted(read - documented),
                                'in docs/KNOBS.md, read nowhere': sorted(documented - read)}


def test_only_the_knob_readers_touch_the_environment():
    """getenv appears in two function bodies of capi_common.h and nowhere else; every reader call names its variable literally
    (so the scan above sees it)."""
    for name, text in sources().items():
        code = strip_comments(text)
        uses = re.findall(r'[^\n]*\b(?:secure_)?getenv\b[^\n]*', code)
        if name == 'capi_common.h':
            assert len(uses) == 2 and all(re.search(r'static inline \w[\w \*]* fbbev_env_(int|str)\(', u) for u in uses), uses
        else:
            assert not uses, (name, uses)
        for call in re.finditer(r'\b(%s)\s*\(\s*([^,)]*)' % '|'.join(READERS), code):
            line = code[code.rfind('\n', 0, call.start()) + 1:code.find('\n', call.start())]
            if 'static inline' in line or line.lstrip().startswith('#define'):
                continue                                            # the readers' own definitions
            assert re.fullmatch(r'"FBBEV_\w+"', call.group(2).strip()), (name, line.strip())
