"""The C library's environment switches live in one table (meme_challenge_amd/csrc/switches.h, filled by switches.cpp): the
table, the code that reads the environment and the user-facing list in INTEGRATION.md name the same variables."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'meme_challenge_amd', 'csrc')

SWITCHES = set("""
UNITER_ATTN_B16X UNITER_ATTN_BWD_FUSED UNITER_ATTN_PRIO UNITER_ATTN_SPLIT UNITER_ATTN_X3 UNITER_ATTN_X3_LAB UNITER_B16_PERSIST
UNITER_B16_RIDERS UNITER_DCTX_SPLIT UNITER_EMBED_BWD_PAR UNITER_GATHER_EX UNITER_GELU_D UNITER_GEMM_SK UNITER_HIDDEN_PREGEN
UNITER_IMG_SK UNITER_KEEP_PREGEN UNITER_LNB_ROWS UNITER_LNB_WAVES UNITER_MAIN_PRIO UNITER_MAIN_PRIO_BF16 UNITER_MAIN_PRIO_X3
UNITER_WGRAD_CFG UNITER_WGRAD_GROUP UNITER_WGRAD_GROUP_F32 UNITER_WGRAD_GROUP_F32_SLOTS UNITER_WGRAD_GROUP_WGS UNITER_WGRAD_SLABS
UNITER_WGRAD_SLOTS UNITER_WGRAD_SLOTS_F32 UNITER_WGRAD_WHOLE UNITER_WGRAD_X3_WGS UNITER_X3_192 UNITER_X3_BALANCED UNITER_X3_BAND_H
UNITER_X3_CFG UNITER_X3_CFG_FFN_UP_FWD UNITER_X3_RIDERS UNITER_X3_WGRAD_CFG UNITER_X3_WIDE
""".split())


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_switch_table_reader_and_document_name_the_same_variables():
    assert len(SWITCHES) == 39
    # switches.h: the comment above each declaration starts with the variable's name
    declared = re.findall(r'^\s*// (UNITER_[A-Z0-9_]+) \(', _read(CSRC, 'switches.h'), flags=re.M)
    assert len(declared) == len(set(declared)), 'a switch is declared twice in switches.h'
    assert set(declared) == SWITCHES
    # switches.cpp: every declared switch is read, by a string literal, exactly once -- and nothing else is
    read = re.findall(r'"(UNITER_[A-Z0-9_]+)"', _read(CSRC, 'switches.cpp'))
    assert sorted(read) == sorted(SWITCHES)
    doc = _read(REPO, 'INTEGRATION.md')
    missing = sorted(n for n in SWITCHES if not re.search(r'\b%s\b' % n, doc))
    assert not missing, 'not in INTEGRATION.md: %s' % missing


def test_only_the_switch_table_reads_the_environment():
    readers = sorted(f for f in os.listdir(CSRC) if 'getenv' in _read(CSRC, f))
    assert readers == ['switches.cpp']
