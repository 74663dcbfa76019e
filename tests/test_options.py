"""The options of a context: one table (sella_amd/csrc/options.h) behind sella_ctx_set_option / sella_ctx_get_option /
sella_option_name, and `Context.options(...)` as the only way tests and tools override them.  PINNED is a literal copy of
what the library did BEFORE the table existed — every default, and for every option a few probe values with what the
hand-written setter made of them — recorded from that setter (a throw-away getter added to a copy of it, the same probes
on the emulator build), not from options.h: changing a default or a rule means changing this table too, visibly."""
import os
import re

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, 'sella_amd', 'csrc')
E = 'error'
BIG = 1 << 40
BOOL = {-BIG: 1, -1: 1, 0: 0, 1: 1, 2: 1, BIG: 1}
# name: (default, {value given to set_option: value stored, or E for SELLA_E_INVALID})
PINNED = {
    'gemv_rw': (0, {-1: E, 0: 0, 1: 1, 2: 2, 3: E, 4: 4, 5: E, 8: E}),
    'eigh_leaf': (16, {-1: E, 1: E, 2: 2, 16: 16, 64: 64, 65: E, BIG: E}),
    'eigh_symv_tr': (64, {0: E, 63: E, 64: 64, 65: E, 127: E, 128: 128, 129: E, 256: E}),
    'eigh_symv_min': (5120, {-BIG: E, -1: E, 0: 0, 1: 1, 5120: 5120, BIG: BIG}),
    'eigh_nb': (16, {-1: E, 0: E, 1: 1, 64: 64, 65: E}),
    'panel_rows': (0, {-1: E, 0: 0, 1: E, 16: 16, 17: E, 32: 32, 48: 48, 64: 64, 65: E, 128: E}),
    'eigh_tail_lds': (128, {-BIG: 0, -1: 0, 0: 0, 1: 1, 128: 128, 129: 129, BIG: BIG}),
    'eigh_wy_nb64_min': (2560, {-BIG: -BIG, -1: -1, 0: 0, 3: 3, BIG: BIG}),
    'eigh_wy_rows': (16, {-BIG: -BIG, -1: -1, 0: 0, 3: 3, BIG: BIG}),
    'eigh_wy_waves': (4, {-BIG: -BIG, -1: -1, 0: 0, 3: 3, BIG: BIG}),
    'h2d_kernel_min': (16384, {-5: 0, -1: 0, 0: 0, 1: 1, 16384: 16384, BIG: BIG}),
    'eigh_wy_strip': (1, {-BIG: -BIG, -1: -1, 0: 0, 3: 3, BIG: BIG}),
    'panel_small': (2048, {-5: 0, -1: 0, 0: 0, 1: 1, 16384: 16384, BIG: BIG}),
    'eigh_upd_max': (1024, {-1: 0, 0: 0, 1024: 1024, 8127: 8127, 8128: 8128, 8129: 8128, 16384: 8128, BIG: 8128}),
    'eigh_upd_rows': (0, {-1: E, 0: 0, 1: E, 2: 2, 3: E, 4: 4, 8: 8, 16: E}),
    'eigh_upd_nt': (512, {0: E, 64: E, 127: E, 128: 128, 129: E, 256: 256, 512: 512, 1024: E}),
    'emt_hcap': (8, {-BIG: -BIG, -1: -1, 0: 0, 3: 3, BIG: BIG}),
    'gs_small': (2048, {-1: 0, 0: 0, 1: 1, 2047: 2047, 2048: 2048, 2049: 2048, BIG: 2048}),
}
PINNED.update({name: (1, BOOL) for name in (
    'gemm_mfma gemm_tile128 panel_mfma eigh_wy_mfma dav_fuse_scale dav_poll lr_cholqr eigh_dc_pipeline eigh_gemv_flat '
    'rank2k_fixed rs_fast lr_dev rank2k_stream dav_rotate_fused bd_early_matvec bd_pipeline eigh_wy_overlap '
    'rs_batch_result lr_pipe lr_chain rs_hint rs_batch').split()})
PINNED.update({name: (0, BOOL) for name in 'host_scalars dav_zero_copy lr_overlap'.split()})
# no caller was left and the default never selected the alternative: retired with the table
RETIRED = ['eigh_upd_r4_min', 'eigh_upd_r8_min', 'eigh_symv_tri', 'rs_poll']


def test_names_are_unique_and_round_trip(ctx):
    names = ctx.option_names()
    assert len(names) == len(set(names))
    assert sorted(names) == sorted(PINNED)
    for name in names:
        value = ctx.get_option(name)
        ctx.set_option(name, value)
        assert ctx.get_option(name) == value, name


def test_defaults_are_the_pinned_ones(ctx):
    """On a context of the test's own (the `ctx` fixture has switched rs_batch off on the emulator)."""
    from sella_amd import device
    fresh = device.Context(0)
    try:
        assert {name: fresh.get_option(name) for name in fresh.option_names()} == {k: v[0] for k, v in PINNED.items()}
    finally:
        fresh.close()


@pytest.mark.parametrize('name', sorted(PINNED))
def test_setter_rule_is_the_pinned_one(ctx, name):
    from sella_amd._lib import SellaHipError
    before = ctx.get_option(name)
    try:
        for value, expected in PINNED[name][1].items():
            if expected == E:
                start = ctx.get_option(name)
                with pytest.raises(SellaHipError):
                    ctx.set_option(name, value)
                assert ctx.get_option(name) == start, (name, value)        # a rejected value changes nothing
            else:
                ctx.set_option(name, value)
                assert ctx.get_option(name) == expected, (name, value)
    finally:
        ctx.set_option(name, before)


def test_scoped_override_puts_back_what_it_found(ctx):
    from sella_amd._lib import SellaHipError
    with ctx.options(eigh_nb=8):                                 # 8 is not the default: it must come back, not 16
        with ctx.options(eigh_nb=4, gs_small=5000, rs_batch=1 - ctx.get_option('rs_batch')) as same:
            assert same is ctx
            assert (ctx.get_option('eigh_nb'), ctx.get_option('gs_small')) == (4, 2048)     # through the setter's rule
        assert ctx.get_option('eigh_nb') == 8
        with pytest.raises(RuntimeError, match='inside'):
            with ctx.options(eigh_nb=32, eigh_leaf=4):
                assert (ctx.get_option('eigh_nb'), ctx.get_option('eigh_leaf')) == (32, 4)
                raise RuntimeError('inside')
        assert (ctx.get_option('eigh_nb'), ctx.get_option('eigh_leaf')) == (8, PINNED['eigh_leaf'][0])
        # a rejected value or an unknown name: nothing stays changed, the body does not run
        for bad in (dict(eigh_nb=2, eigh_leaf=1000), dict(eigh_nb=2, no_such_option=1)):
            with pytest.raises(SellaHipError):
                with ctx.options(**bad):
                    raise AssertionError('body ran')
            assert ctx.get_option('eigh_nb') == 8
    assert ctx.get_option('eigh_nb') == PINNED['eigh_nb'][0]
    assert ctx.get_option('rs_batch') == (0 if ctx.backend == 'emu' else 1)      # conftest.make_context's setting


def test_retired_and_unknown_names_are_rejected(ctx):
    from sella_amd._lib import SellaHipError
    for name in RETIRED + ['no_such_option', '']:
        assert name not in ctx.option_names()
        for call in (lambda: ctx.set_option(name, 1), lambda: ctx.get_option(name)):
            with pytest.raises(SellaHipError, match=f"unknown option '{name}'"):
                call()


def test_one_table_entry_per_name_and_one_writer(ctx):
    """Every option is one SELLA_OPTION line of options.h, and nothing but the setter (context.hip) assigns to an
    option: a call that needs another behaviour for its own length keeps it in run state of the context."""
    table = open(os.path.join(CSRC, 'options.h')).read()
    entries = re.findall(r'^SELLA_OPTION\(\s*(\w+)\s*,', table, flags=re.M)
    assert sorted(entries) == sorted(ctx.option_names())
    for name in ctx.option_names():
        assert len(re.findall(r'\bSELLA_OPTION\(\s*%s\s*,' % name, table)) == 1, name
    assign = re.compile(r'\bopt\.\w+\s*(?:(?:[-+*/%&|^]|<<|>>)?=(?!=)|\+\+|--)|(?:\+\+|--)\s*[\w>.-]*\bopt\.')
    assert assign.search('c->opt.host_scalars = 1;') and assign.search('c->opt.x |= 2') and assign.search('c.opt.n++')
    assert not assign.search('if (c->opt.a == 1 && c->opt.b <= 2) x = c->opt.c;')
    writers = [f for f in sorted(os.listdir(CSRC)) if f.endswith(('.hip', '.h')) and f != 'context.hip'
               and any(assign.search(line.split('//')[0]) for line in open(os.path.join(CSRC, f)))]
    assert not writers, writers
