"""vfs_amd/knobs.py: the one table of the Python side's VFS_* environment variables and its accessors.
  * the defaults are pinned to what the read sites used before the table existed;
  * no module of vfs_amd/ but knobs.py (and build.py: HIPCC, EMU_CXX) reads the environment, every name an accessor is called with
    is a row of the matching kind, and every row has a reader;
  * the accessors give what the hand-written expressions they replaced gave;
  * the Knobs section of INTEGRATION.md lists exactly the `product` rows."""
import glob
import os
import re

import pytest

from vfs_amd import knobs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> default of the read site(s) at the commit before the table (None: read without a default).  A changed default shows here.
DEFAULTS = {
    'VFS_TAPE': '1', 'VFS_GRAPHS': '0', 'VFS_GC_FREEZE': '0', 'VFS_SIDE_STREAM': '1', 'VFS_MAIN_PRIO': None, 'VFS_FAST_TRAIN_STEP': '1',
    'VFS_LAZY_LOG': '1', 'VFS_LOG_ASYNC': '1',
    'VFS_FIN_FUSE': '1', 'VFS_FIN_MAX_ROWS': '128', 'VFS_FIN_XCHG': '0', 'VFS_RAW_STATS': '1', 'VFS_HEAD_FUSE': '1', 'VFS_BN_FUSE': '1',
    'VFS_MASK_BITS': '1', 'VFS_MASK_ADD': '1',
    'VFS_BNACT_FUSE': '1', 'VFS_BNACT_FUSE_MB': '16', 'VFS_BNACT_FUSE_1X1': '1', 'VFS_BNACT_FUSE_1X1_MB': '16', 'VFS_BNACT_FUSE_SMALL': '0',
    'VFS_WGRAD_TB': '192', 'VFS_WGRAD_TBG': None,      # (unset: wgrad_splits' target_blocks argument, 192 unless the caller says otherwise)
    'VFS_WGRAD_TBG_SMALL': None, 'VFS_WGRAD_TBG_DEEP': None, 'VFS_WGRAD_BATCH': '0', 'VFS_STEM_FUSED': '1', 'VFS_STEM_WGRAD_BLOCKS': '1536',
    'VFS_FAST_PACK': '1',
    'VFS_FORCE_COLLECTIVES': None, 'VFS_SYNCBN_P2P': '1', 'VFS_P2P_SPIN': '2147483648', 'VFS_P2P_CHECK_EVERY': '50', 'VFS_GRAD_BF16': '0',
    'VFS_DDP_AVG': '1', 'VFS_DDP_SIDE': '1',
    'VFS_EVAL_PRECISION': 'fp32', 'VFS_LP_TWO_PASS': '1', 'VFS_LP2_ENTRIES': '0',
    'VFS_HIP_LIB': None, 'VFS_OPTS': '', 'VFS_TRACE_CALLS': None, 'VFS_DEBUG_SKIP': '', 'VFS_DEBUG_NOMASK': None,
}

ACCESSOR_OF_KIND = {'flag': 'flag', 'int': 'integer', 'float': 'number', 'str': 'text', 'choice': 'text', 'optional int': 'optional',
                    'list': 'items'}


def test_defaults_are_pinned():
    assert {name: row[0] for name, row in knobs.TABLE.items()} == DEFAULTS


def test_rows_are_well_formed():
    for name, (default, kind, cls, doc) in knobs.TABLE.items():
        assert re.fullmatch(r'VFS_[A-Z0-9_]+', name)
        assert default is None or isinstance(default, str), name
        assert kind.split(':')[0] in ACCESSOR_OF_KIND, (name, kind)
        assert cls in ('product', 'ab', 'debug'), (name, cls)
        assert doc and '|' not in doc and '\n' not in doc, name      # (one line, one Markdown cell)
        if kind.startswith('choice'):
            assert default is None or default in [v.strip() for v in kind.split(':')[1].split(',')], name


def _sources():
    paths = sorted(glob.glob(os.path.join(REPO, 'vfs_amd', '*.py')))
    assert len(paths) > 20
    return {os.path.basename(p): open(p).read() for p in paths if os.path.basename(p) not in ('knobs.py', 'build.py')}


def test_no_stray_reads_and_no_dead_rows():
    used = set()
    for fname, src in _sources().items():
        assert 'os.environ' not in src and 'getenv' not in src, fname
        # every accessor call names its knob(s) literally, each a row of the kind the accessor parses
        for acc, args in re.findall(r'knobs\.(flag|integer|number|text|optional|items)\(([^()]*)', src):
            names = re.findall(r"'(VFS_[A-Z0-9_]+)'", args)
            assert names, (fname, acc, args)
            for name in names:
                assert name in knobs.TABLE, (fname, name)
                assert ACCESSOR_OF_KIND[knobs.TABLE[name][1].split(':')[0]] == acc, (fname, name, acc)
                used.add(name)
        # ... and nothing else in the file spells a whole VFS_* name as a string of its own
        assert set(re.findall(r"""['"](VFS_[A-Z0-9_]+)['"]""", src)) <= set(knobs.TABLE), fname
    assert used == set(knobs.TABLE), sorted(set(knobs.TABLE) - used)


def _old(name, default=None):
    return os.environ.get(name, default)


# one knob of each kind: (accessor, name, the expression the read site held before, values to try - None: unset)
PARSING = [
    (knobs.flag, 'VFS_MASK_BITS', lambda: _old('VFS_MASK_BITS', '1') == '1', [None, '1', '0', 'true', '']),
    (knobs.flag, 'VFS_DEBUG_NOMASK', lambda: _old('VFS_DEBUG_NOMASK') == '1', [None, '1', '0', 'true']),
    (knobs.integer, 'VFS_FIN_MAX_ROWS', lambda: int(_old('VFS_FIN_MAX_ROWS', '128')), [None, '64', ' 7 ', '0']),
    (knobs.number, 'VFS_BNACT_FUSE_MB', lambda: float(_old('VFS_BNACT_FUSE_MB', '16')), [None, '0', '2.5', '1e3']),
    (knobs.text, 'VFS_HIP_LIB', lambda: _old('VFS_HIP_LIB'), [None, '', '/somewhere/libvfs_hip.so']),
    (knobs.text, 'VFS_SYNCBN_P2P', lambda: _old('VFS_SYNCBN_P2P', '1'), [None, '0', '1', 'force']),
    (knobs.text, 'VFS_MAIN_PRIO', lambda: _old('VFS_MAIN_PRIO'), [None, '0', '1']),
    (knobs.optional, 'VFS_WGRAD_TBG_SMALL', lambda: int(os.environ['VFS_WGRAD_TBG_SMALL']) if 'VFS_WGRAD_TBG_SMALL' in os.environ else None,
     [None, '96', '0']),
    (knobs.items, 'VFS_DEBUG_SKIP', lambda: list(filter(None, _old('VFS_DEBUG_SKIP', '').split(','))), [None, '', 'bn_act', 'bn_act,,sgd,']),
]


@pytest.mark.parametrize('accessor,name,old,values', PARSING, ids=[f'{c[0].__name__}-{c[1]}' for c in PARSING])
def test_accessors_parse_like_the_read_sites_did(accessor, name, old, values, monkeypatch):
    for v in values:      # (read at the moment of the call: no import or cache in between)
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
        got, want = accessor(name), old()
        assert got == want and type(got) is type(want), (name, v, got, want)


def test_every_kind_has_a_parsing_case():
    assert {ACCESSOR_OF_KIND[row[1].split(':')[0]] for row in knobs.TABLE.values()} == {c[0].__name__ for c in PARSING}
    assert {row[1].split(':')[0] for row in knobs.TABLE.values()} == set(ACCESSOR_OF_KIND)


def test_flag_is_on_for_the_string_1_only(monkeypatch):
    monkeypatch.setenv('VFS_GRAPHS', 'true')
    assert knobs.flag('VFS_GRAPHS') is False
    monkeypatch.setenv('VFS_GRAPHS', '1')
    assert knobs.flag('VFS_GRAPHS') is True
    monkeypatch.delenv('VFS_GRAPHS')
    assert knobs.flag('VFS_GRAPHS') is False and knobs.flag('VFS_TAPE') is True      # the defaults


def test_choice_knob_values(monkeypatch):
    for v in ('0', '1', 'force'):
        monkeypatch.setenv('VFS_SYNCBN_P2P', v)
        assert knobs.text('VFS_SYNCBN_P2P') == v
    monkeypatch.delenv('VFS_SYNCBN_P2P')
    assert knobs.text('VFS_SYNCBN_P2P') == '1'


def test_optional_ints_are_none_when_unset(monkeypatch):
    for name in ('VFS_WGRAD_TBG', 'VFS_WGRAD_TBG_SMALL', 'VFS_WGRAD_TBG_DEEP'):
        monkeypatch.delenv(name, raising=False)
        assert knobs.optional(name) is None and knobs.optional(name, 12) == 12
        monkeypatch.setenv(name, '48')
        assert knobs.optional(name) == 48 and knobs.optional(name, 12) == 48


def test_empty_library_path_falls_back_to_the_built_library(monkeypatch):
    from vfs_amd import _lib
    monkeypatch.setattr(_lib, 'VfsLib', lambda path: path)      # (get_lib's answer is then the path it would load)
    for v, want in ((None, _lib.LIB_PATH), ('', _lib.LIB_PATH), ('/somewhere/libvfs_hip.so', '/somewhere/libvfs_hip.so')):
        monkeypatch.delenv('VFS_HIP_LIB', raising=False) if v is None else monkeypatch.setenv('VFS_HIP_LIB', v)
        monkeypatch.setattr(_lib, '_LIB', None)
        assert _lib.get_lib() == want


def test_unknown_name_is_a_key_error(monkeypatch):
    monkeypatch.setenv('VFS_MASK_BIT', '0')      # (set or not: a name outside the table is refused)
    for accessor in (knobs.flag, knobs.integer, knobs.number, knobs.text, knobs.optional, knobs.items):
        with pytest.raises(KeyError):
            accessor('VFS_MASK_BIT')


@pytest.mark.parametrize('accessor,name', [(knobs.integer, 'VFS_WGRAD_TB'), (knobs.number, 'VFS_BNACT_FUSE_1X1_MB'),
                                           (knobs.optional, 'VFS_WGRAD_TBG_DEEP')])
def test_unparsable_number_is_a_value_error_that_names_the_knob(accessor, name, monkeypatch):
    for v in ('many', ''):
        monkeypatch.setenv(name, v)
        with pytest.raises(ValueError, match=name):
            accessor(name)


def test_wgrad_target_knob_overrides_the_callers_target_only_when_set(monkeypatch):
    """VFS_WGRAD_TBG had the caller's target_blocks as its default: unset, the argument holds; set, the knob wins"""
    from vfs_amd.packing import wgrad_splits
    shape = (1 << 16, 256, 2304)
    for name in ('VFS_WGRAD_TBG', 'VFS_WGRAD_TBG_SMALL', 'VFS_WGRAD_TBG_DEEP'):
        monkeypatch.delenv(name, raising=False)
    few, many = wgrad_splits(*shape, target_blocks=36), wgrad_splits(*shape, target_blocks=144)
    assert few != many and wgrad_splits(*shape) == wgrad_splits(*shape, target_blocks=192)
    monkeypatch.setenv('VFS_WGRAD_TBG', '144')
    assert wgrad_splits(*shape, target_blocks=36) == many
    monkeypatch.setenv('VFS_WGRAD_TBG_DEEP', '36')      # 18 x 2 tiles: the deep-layer target applies on top
    assert wgrad_splits(*shape, target_blocks=144) == few


def test_integration_md_lists_the_product_knobs():
    text = open(os.path.join(REPO, 'INTEGRATION.md')).read()
    section = re.search(r'^## [^\n]*Knobs[^\n]*\n(.*?)(?=^## |\Z)', text, flags=re.S | re.M).group(1)
    listed = set(re.findall(r'^\| `(VFS_[A-Z0-9_]+)`', section, flags=re.M))
    assert listed == {name for name, row in knobs.TABLE.items() if row[2] == 'product'}
    assert 'python -m vfs_amd.knobs' in section
