"""Masked-edit configuration keys, characterised: what the five ``config.*_options`` functions return or refuse, and the directory name
``output_suffix`` forms, for literal tables of configurations.  The expected values were recorded from the functions themselves (not
written by hand) before the key handling moved into ``anyv2v_amd/masked_edit.py``; they hold across that move unchanged.  CPU only, no
library."""
import pytest

from anyv2v_amd import config as cfgmod
from anyv2v_amd.config import OmegaConf
from anyv2v_amd.run_group_pnp_edit import output_suffix

nan, inf = float("nan"), float("inf")
BASE = dict(n_steps=50, cfg=9.0, pnp_f_t=0.2, pnp_spatial_attn_t=0.2, pnp_temp_attn_t=0.5)
S = "ddim_init_latents_t_idx_1_nsteps_50_cfg_9.0_pnpf0.2_pnps0.2_pnpt0.5"   # ``output_suffix(BASE, 1)``
FUNCS = ("masked_edit_options", "first_frame_mask_options", "track_options", "auto_mask_options", "composite_options")

# (keys, masked_edit_options, first_frame_mask_options, track_options, auto_mask_options, composite_options, output_suffix(config, 1))
ACCEPTED = [
    ({},
     None, None, None, None, None,
     S),
    ({'edit_mask_auto': False, 'edit_mask_first_frame': False, 'edit_mask_track': False, 'edit_mask_composite': False, 'edit_mask_path': None},
     None, None, None, None, None,
     S),
    ({'edit_mask_path': 'masks/hat.png'},
     ('masks/hat.png', 0, 0.0), None, None, None, None,
     S + '_mask-hat'),
    ({'edit_mask_path': 'masks/hat.png', 'edit_mask_grow': 2, 'edit_mask_feather': 1.5},
     ('masks/hat.png', 2, 1.5), None, None, None, None,
     S + '_mask-hat_grow2_feather1.5'),
    ({'edit_mask_path': 'demo/clip/masks/'},
     ('demo/clip/masks/', 0, 0.0), None, None, None, None,
     S + '_mask-masks'),
    ({'edit_mask_path': 'hat.png', 'edit_mask_grow': 8, 'edit_mask_feather': 8},
     ('hat.png', 8, 8.0), None, None, None, None,
     S + '_mask-hat_grow8_feather8.0'),
    ({'edit_mask_path': 'hat.png', 'edit_mask_grow': 2.0, 'edit_mask_feather': 0},
     ('hat.png', 2, 0.0), None, None, None, None,
     S + '_mask-hat_grow2'),
    ({'edit_mask_auto': True},
     None, None, None, {'maps': 10, 'grow': 0, 'feather': 0.0, 'strength': 0.5, 'ratio': 3.0, 'threshold': 0.5}, None,
     S + '_mask-auto'),
    ({'edit_mask_auto': True, 'edit_mask_grow': 1, 'edit_mask_feather': 0.5},
     None, None, None, {'maps': 10, 'grow': 1, 'feather': 0.5, 'strength': 0.5, 'ratio': 3.0, 'threshold': 0.5}, None,
     S + '_mask-auto_grow1_feather0.5'),
    ({'edit_mask_auto': True, 'edit_mask_auto_maps': 3, 'edit_mask_auto_strength': 0.8, 'edit_mask_auto_ratio': 2, 'edit_mask_auto_threshold': 0.25},
     None, None, None, {'maps': 3, 'grow': 0, 'feather': 0.0, 'strength': 0.8, 'ratio': 2.0, 'threshold': 0.25}, None,
     S + '_mask-auto_maps3_strength0.8_ratio2.0_threshold0.25'),
    ({'edit_mask_auto': True, 'edit_mask_auto_maps': 4.0, 'edit_mask_auto_strength': 1},
     None, None, None, {'maps': 4, 'grow': 0, 'feather': 0.0, 'strength': 1.0, 'ratio': 3.0, 'threshold': 0.5}, None,
     S + '_mask-auto_maps4_strength1.0'),
    ({'edit_mask_first_frame': True},
     None, {'threshold': 24, 'min_count': 8, 'grow': 0, 'feather': 0.0}, None, None, None,
     S + '_mask-ff'),
    ({'edit_mask_first_frame': True, 'edit_mask_grow': 3, 'edit_mask_feather': 2.25},
     None, {'threshold': 24, 'min_count': 8, 'grow': 3, 'feather': 2.25}, None, None, None,
     S + '_mask-ff_grow3_feather2.25'),
    ({'edit_mask_first_frame': True, 'edit_mask_first_frame_threshold': 30, 'edit_mask_first_frame_min_count': 4},
     None, {'threshold': 30, 'min_count': 4, 'grow': 0, 'feather': 0.0}, None, None, None,
     S + '_mask-ff_threshold30_min_count4'),
    ({'edit_mask_first_frame': True, 'edit_mask_first_frame_threshold': 0, 'edit_mask_first_frame_min_count': 1},
     None, {'threshold': 0, 'min_count': 1, 'grow': 0, 'feather': 0.0}, None, None, None,
     S + '_mask-ff_threshold0_min_count1'),
    ({'edit_mask_first_frame': True, 'edit_mask_first_frame_threshold': 255, 'edit_mask_first_frame_min_count': 64},
     None, {'threshold': 255, 'min_count': 64, 'grow': 0, 'feather': 0.0}, None, None, None,
     S + '_mask-ff_threshold255_min_count64'),
    ({'edit_mask_first_frame': True, 'edit_mask_track': True},
     None, {'threshold': 24, 'min_count': 8, 'grow': 0, 'feather': 0.0}, {'radius': 16, 'median': True}, None, None,
     S + '_mask-ff-track'),
    ({'edit_mask_path': 'demo/clip/hat.png', 'edit_mask_track': True},
     ('demo/clip/hat.png', 0, 0.0), None, {'radius': 16, 'median': True}, None, None,
     S + '_mask-hat-track'),
    ({'edit_mask_first_frame': True, 'edit_mask_track': True, 'edit_mask_track_radius': 8},
     None, {'threshold': 24, 'min_count': 8, 'grow': 0, 'feather': 0.0}, {'radius': 8, 'median': True}, None, None,
     S + '_mask-ff-track_radius8'),
    ({'edit_mask_first_frame': True, 'edit_mask_track': True, 'edit_mask_track_median': False},
     None, {'threshold': 24, 'min_count': 8, 'grow': 0, 'feather': 0.0}, {'radius': 16, 'median': False}, None, None,
     S + '_mask-ff-track_nomedian'),
    ({'edit_mask_path': 'hat.png', 'edit_mask_track': True, 'edit_mask_track_radius': 32, 'edit_mask_track_median': False, 'edit_mask_feather': 1.0},
     ('hat.png', 0, 1.0), None, {'radius': 32, 'median': False}, None, None,
     S + '_mask-hat-track_radius32_nomedian_feather1.0'),
    ({'edit_mask_first_frame': True, 'edit_mask_track': True, 'edit_mask_track_radius': 0, 'edit_mask_track_median': True},
     None, {'threshold': 24, 'min_count': 8, 'grow': 0, 'feather': 0.0}, {'radius': 0, 'median': True}, None, None,
     S + '_mask-ff-track_radius0'),
    ({'edit_mask_path': 'hat.png', 'edit_mask_composite': True},
     ('hat.png', 0, 0.0), None, None, None, {'grow_px': 0, 'feather_px': 0.0, 'match_color': False},
     S + '_mask-hat_comp'),
    ({'edit_mask_auto': True, 'edit_mask_composite': True},
     None, None, None, {'maps': 10, 'grow': 0, 'feather': 0.0, 'strength': 0.5, 'ratio': 3.0, 'threshold': 0.5}, {'grow_px': 0, 'feather_px': 0.0, 'match_color': False},
     S + '_mask-auto_comp'),
    ({'edit_mask_first_frame': True, 'edit_mask_composite': True},
     None, {'threshold': 24, 'min_count': 8, 'grow': 0, 'feather': 0.0}, None, None, {'grow_px': 0, 'feather_px': 0.0, 'match_color': False},
     S + '_mask-ff_comp'),
    ({'edit_mask_auto': True, 'edit_mask_composite': True, 'edit_mask_composite_grow': 4, 'edit_mask_composite_feather': 2.5, 'edit_mask_match_color': True},
     None, None, None, {'maps': 10, 'grow': 0, 'feather': 0.0, 'strength': 0.5, 'ratio': 3.0, 'threshold': 0.5}, {'grow_px': 4, 'feather_px': 2.5, 'match_color': True},
     S + '_mask-auto_comp_grow4_feather2.5_match'),
    ({'edit_mask_path': 'hat.png', 'edit_mask_composite': True, 'edit_mask_composite_grow': 64, 'edit_mask_composite_feather': 16, 'edit_mask_match_color': False},
     ('hat.png', 0, 0.0), None, None, None, {'grow_px': 64, 'feather_px': 16.0, 'match_color': False},
     S + '_mask-hat_comp_grow64_feather16.0'),
    ({'edit_mask_first_frame': True, 'edit_mask_first_frame_threshold': 30, 'edit_mask_grow': 2, 'edit_mask_track': True, 'edit_mask_track_radius': 8, 'edit_mask_track_median': False, 'edit_mask_composite': True, 'edit_mask_composite_grow': 3, 'edit_mask_match_color': True},
     None, {'threshold': 30, 'min_count': 8, 'grow': 2, 'feather': 0.0}, {'radius': 8, 'median': False}, None, {'grow_px': 3, 'feather_px': 0.0, 'match_color': True},
     S + '_mask-ff_threshold30-track_radius8_nomedian_grow2_comp_grow3_match'),
    ({'edit_mask_auto': True, 'edit_mask_auto_threshold': 0.75, 'edit_mask_grow': 2, 'edit_mask_feather': 1.5, 'edit_mask_composite': True, 'edit_mask_composite_feather': 1.0},
     None, None, None, {'maps': 10, 'grow': 2, 'feather': 1.5, 'strength': 0.5, 'ratio': 3.0, 'threshold': 0.75}, {'grow_px': 0, 'feather_px': 1.0, 'match_color': False},
     S + '_mask-auto_threshold0.75_grow2_feather1.5_comp_feather1.0'),
]

# (the function that raises, keys, the complete message)
REFUSED = [
    ('masked_edit_options', {'edit_mask_path': 'm.png', 'edit_mask_auto': True},
     'edit_mask_auto together with edit_mask_path: the mask is either generated or loaded'),
    ('auto_mask_options', {'edit_mask_path': 'm.png', 'edit_mask_auto': True},
     'edit_mask_auto together with edit_mask_path: the mask is either generated or loaded'),
    ('masked_edit_options', {'edit_mask_path': 'm.png', 'edit_mask_first_frame': True},
     'edit_mask_first_frame together with edit_mask_path: the mask is either derived from the first frames or loaded'),
    ('first_frame_mask_options', {'edit_mask_path': 'm.png', 'edit_mask_first_frame': True},
     'edit_mask_first_frame together with edit_mask_path: the mask is either derived from the first frames or loaded'),
    ('first_frame_mask_options', {'edit_mask_first_frame': True, 'edit_mask_auto': True},
     'edit_mask_first_frame together with edit_mask_auto: the mask is either derived from the first frames or generated'),
    ('auto_mask_options', {'edit_mask_first_frame': True, 'edit_mask_auto': True},
     'edit_mask_first_frame together with edit_mask_auto: the mask is either derived from the first frames or generated'),
    ('masked_edit_options', {'edit_mask_path': 'm.png', 'edit_mask_auto': True, 'edit_mask_first_frame': True},
     'edit_mask_auto together with edit_mask_path: the mask is either generated or loaded'),
    ('auto_mask_options', {'edit_mask_auto_maps': 3},
     'edit_mask_auto_maps without edit_mask_auto: there is no automatic mask to tune'),
    ('auto_mask_options', {'edit_mask_auto_strength': 0.8},
     'edit_mask_auto_strength without edit_mask_auto: there is no automatic mask to tune'),
    ('auto_mask_options', {'edit_mask_auto_ratio': 2.0},
     'edit_mask_auto_ratio without edit_mask_auto: there is no automatic mask to tune'),
    ('auto_mask_options', {'edit_mask_auto': False, 'edit_mask_auto_threshold': 0.25},
     'edit_mask_auto_threshold without edit_mask_auto: there is no automatic mask to tune'),
    ('first_frame_mask_options', {'edit_mask_first_frame_threshold': 30},
     'edit_mask_first_frame_threshold without edit_mask_first_frame: there is no first-frame mask to tune'),
    ('first_frame_mask_options', {'edit_mask_first_frame': False, 'edit_mask_first_frame_min_count': 4},
     'edit_mask_first_frame_min_count without edit_mask_first_frame: there is no first-frame mask to tune'),
    ('track_options', {'edit_mask_first_frame': True, 'edit_mask_track_radius': 8},
     'edit_mask_track_radius without edit_mask_track: there is no tracking to tune'),
    ('track_options', {'edit_mask_first_frame': True, 'edit_mask_track': False, 'edit_mask_track_median': False},
     'edit_mask_track_median without edit_mask_track: there is no tracking to tune'),
    ('composite_options', {'edit_mask_auto': True, 'edit_mask_composite_grow': 4},
     'edit_mask_composite_grow without edit_mask_composite: there is no composite to shape'),
    ('composite_options', {'edit_mask_auto': True, 'edit_mask_composite_feather': 1.0},
     'edit_mask_composite_feather without edit_mask_composite: there is no composite to shape'),
    ('composite_options', {'edit_mask_auto': True, 'edit_mask_composite': False, 'edit_mask_match_color': True},
     'edit_mask_match_color without edit_mask_composite: there is no composite to shape'),
    ('masked_edit_options', {'edit_mask_grow': 2},
     'edit_mask_grow / edit_mask_feather without edit_mask_path: there is no mask to grow or feather'),
    ('masked_edit_options', {'edit_mask_feather': 1.0},
     'edit_mask_grow / edit_mask_feather without edit_mask_path: there is no mask to grow or feather'),
    ('track_options', {'edit_mask_track': True, 'edit_mask_auto': True},
     'edit_mask_track together with edit_mask_auto: the generated mask already has every frame'),
    ('track_options', {'edit_mask_track': True},
     'edit_mask_track without edit_mask_first_frame or edit_mask_path: there is no frame-0 mask to carry'),
    ('composite_options', {'edit_mask_composite': True},
     'edit_mask_composite without edit_mask_path or edit_mask_auto: there is no mask to composite by'),
    ('composite_options', {'edit_mask_first_frame': False, 'edit_mask_composite': True},
     'edit_mask_composite without edit_mask_path or edit_mask_auto: there is no mask to composite by'),
    ('masked_edit_options', {'edit_mask_path': 'm.png', 'edit_mask_grow': 9},
     'edit_mask_grow=9: an integer, 0 <= edit_mask_grow <= 8'),
    ('masked_edit_options', {'edit_mask_path': 'm.png', 'edit_mask_grow': -1},
     'edit_mask_grow=-1: an integer, 0 <= edit_mask_grow <= 8'),
    ('masked_edit_options', {'edit_mask_path': 'm.png', 'edit_mask_feather': 9},
     'edit_mask_feather=9.0: 0 <= edit_mask_feather <= 8'),
    ('masked_edit_options', {'edit_mask_path': 'm.png', 'edit_mask_feather': -1},
     'edit_mask_feather=-1.0: 0 <= edit_mask_feather <= 8'),
    ('auto_mask_options', {'edit_mask_auto': True, 'edit_mask_grow': 9},
     'edit_mask_grow=9: an integer, 0 <= edit_mask_grow <= 8'),
    ('first_frame_mask_options', {'edit_mask_first_frame': True, 'edit_mask_feather': 8.5},
     'edit_mask_feather=8.5: 0 <= edit_mask_feather <= 8'),
    ('first_frame_mask_options', {'edit_mask_first_frame': True, 'edit_mask_first_frame_threshold': 256},
     'edit_mask_first_frame_threshold=256: an integer, 0 <= edit_mask_first_frame_threshold <= 255'),
    ('first_frame_mask_options', {'edit_mask_first_frame': True, 'edit_mask_first_frame_threshold': -1},
     'edit_mask_first_frame_threshold=-1: an integer, 0 <= edit_mask_first_frame_threshold <= 255'),
    ('first_frame_mask_options', {'edit_mask_first_frame': True, 'edit_mask_first_frame_min_count': 65},
     'edit_mask_first_frame_min_count=65: an integer, 1 <= edit_mask_first_frame_min_count <= 64'),
    ('first_frame_mask_options', {'edit_mask_first_frame': True, 'edit_mask_first_frame_min_count': 0},
     'edit_mask_first_frame_min_count=0: an integer, 1 <= edit_mask_first_frame_min_count <= 64'),
    ('track_options', {'edit_mask_first_frame': True, 'edit_mask_track': True, 'edit_mask_track_radius': 33},
     'edit_mask_track_radius=33: an integer, 0 <= edit_mask_track_radius <= 32'),
    ('track_options', {'edit_mask_first_frame': True, 'edit_mask_track': True, 'edit_mask_track_radius': -1},
     'edit_mask_track_radius=-1: an integer, 0 <= edit_mask_track_radius <= 32'),
    ('composite_options', {'edit_mask_auto': True, 'edit_mask_composite': True, 'edit_mask_composite_grow': 65},
     'edit_mask_composite_grow=65: an integer, 0 <= edit_mask_composite_grow <= 64'),
    ('composite_options', {'edit_mask_auto': True, 'edit_mask_composite': True, 'edit_mask_composite_grow': -1},
     'edit_mask_composite_grow=-1: an integer, 0 <= edit_mask_composite_grow <= 64'),
    ('composite_options', {'edit_mask_auto': True, 'edit_mask_composite': True, 'edit_mask_composite_feather': 17},
     'edit_mask_composite_feather=17.0: 0 <= edit_mask_composite_feather <= 16'),
    ('composite_options', {'edit_mask_auto': True, 'edit_mask_composite': True, 'edit_mask_composite_feather': -1},
     'edit_mask_composite_feather=-1.0: 0 <= edit_mask_composite_feather <= 16'),
    ('auto_mask_options', {'edit_mask_auto': True, 'edit_mask_auto_maps': 0},
     'edit_mask_auto_maps=0: an integer >= 1'),
    ('auto_mask_options', {'edit_mask_auto': True, 'edit_mask_auto_maps': 2147483648},
     'edit_mask_auto_maps=2147483648: an integer >= 1'),
    ('auto_mask_options', {'edit_mask_auto': True, 'edit_mask_auto_strength': 0},
     'edit_mask_auto_strength=0.0: 0 < edit_mask_auto_strength <= 1'),
    ('auto_mask_options', {'edit_mask_auto': True, 'edit_mask_auto_strength': 1.5},
     'edit_mask_auto_strength=1.5: 0 < edit_mask_auto_strength <= 1'),
    ('auto_mask_options', {'edit_mask_auto': True, 'edit_mask_auto_ratio': 0},
     'edit_mask_auto_ratio=0.0: finite and > 0'),
    ('auto_mask_options', {'edit_mask_auto': True, 'edit_mask_auto_ratio': inf},
     'edit_mask_auto_ratio=inf: finite and > 0'),
    ('auto_mask_options', {'edit_mask_auto': True, 'edit_mask_auto_threshold': 0},
     'edit_mask_auto_threshold=0.0: 0 < edit_mask_auto_threshold < 1'),
    ('auto_mask_options', {'edit_mask_auto': True, 'edit_mask_auto_threshold': 1},
     'edit_mask_auto_threshold=1.0: 0 < edit_mask_auto_threshold < 1'),
    ('masked_edit_options', {'edit_mask_path': 'm.png', 'edit_mask_grow': True},
     'edit_mask_grow=True: an integer, 0 <= edit_mask_grow <= 8'),
    ('masked_edit_options', {'edit_mask_path': 'm.png', 'edit_mask_grow': 1.5},
     'edit_mask_grow=1.5: an integer, 0 <= edit_mask_grow <= 8'),
    ('first_frame_mask_options', {'edit_mask_first_frame': True, 'edit_mask_first_frame_threshold': True},
     'edit_mask_first_frame_threshold=True: an integer, 0 <= edit_mask_first_frame_threshold <= 255'),
    ('first_frame_mask_options', {'edit_mask_first_frame': True, 'edit_mask_first_frame_min_count': True},
     'edit_mask_first_frame_min_count=True: an integer, 1 <= edit_mask_first_frame_min_count <= 64'),
    ('first_frame_mask_options', {'edit_mask_first_frame': True, 'edit_mask_first_frame_threshold': 1.5},
     'edit_mask_first_frame_threshold=1.5: an integer, 0 <= edit_mask_first_frame_threshold <= 255'),
    ('track_options', {'edit_mask_first_frame': True, 'edit_mask_track': True, 'edit_mask_track_radius': True},
     'edit_mask_track_radius=True: an integer, 0 <= edit_mask_track_radius <= 32'),
    ('track_options', {'edit_mask_first_frame': True, 'edit_mask_track': True, 'edit_mask_track_radius': 2.5},
     'edit_mask_track_radius=2.5: an integer, 0 <= edit_mask_track_radius <= 32'),
    ('composite_options', {'edit_mask_auto': True, 'edit_mask_composite': True, 'edit_mask_composite_grow': True},
     'edit_mask_composite_grow=True: an integer, 0 <= edit_mask_composite_grow <= 64'),
    ('auto_mask_options', {'edit_mask_auto': True, 'edit_mask_auto_maps': True},
     'edit_mask_auto_maps=True: an integer >= 1'),
    ('auto_mask_options', {'edit_mask_auto': True, 'edit_mask_auto_maps': 2.5},
     'edit_mask_auto_maps=2.5: an integer >= 1'),
    ('masked_edit_options', {'edit_mask_path': 'm.png', 'edit_mask_grow': nan},
     'edit_mask_grow=nan: an integer, 0 <= edit_mask_grow <= 8'),
    ('masked_edit_options', {'edit_mask_path': 'm.png', 'edit_mask_feather': nan},
     'edit_mask_feather=nan: 0 <= edit_mask_feather <= 8'),
    ('first_frame_mask_options', {'edit_mask_first_frame': True, 'edit_mask_first_frame_threshold': nan},
     'edit_mask_first_frame_threshold=nan: an integer, 0 <= edit_mask_first_frame_threshold <= 255'),
    ('track_options', {'edit_mask_first_frame': True, 'edit_mask_track': True, 'edit_mask_track_radius': nan},
     'edit_mask_track_radius=nan: an integer, 0 <= edit_mask_track_radius <= 32'),
    ('composite_options', {'edit_mask_auto': True, 'edit_mask_composite': True, 'edit_mask_composite_grow': nan},
     'edit_mask_composite_grow=nan: an integer, 0 <= edit_mask_composite_grow <= 64'),
    ('composite_options', {'edit_mask_auto': True, 'edit_mask_composite': True, 'edit_mask_composite_feather': nan},
     'edit_mask_composite_feather=nan: 0 <= edit_mask_composite_feather <= 16'),
    ('auto_mask_options', {'edit_mask_auto': True, 'edit_mask_auto_maps': nan},
     'edit_mask_auto_maps=nan: an integer >= 1'),
    ('auto_mask_options', {'edit_mask_auto': True, 'edit_mask_auto_strength': nan},
     'edit_mask_auto_strength=nan: 0 < edit_mask_auto_strength <= 1'),
    ('auto_mask_options', {'edit_mask_auto': True, 'edit_mask_auto_ratio': nan},
     'edit_mask_auto_ratio=nan: finite and > 0'),
    ('auto_mask_options', {'edit_mask_auto': True, 'edit_mask_auto_threshold': nan},
     'edit_mask_auto_threshold=nan: 0 < edit_mask_auto_threshold < 1'),
    ('auto_mask_options', {'edit_mask_auto': 'yes'},
     "edit_mask_auto='yes': true or false"),
    ('masked_edit_options', {'edit_mask_path': 'm.png', 'edit_mask_auto': 1},
     'edit_mask_auto=1: true or false'),
    ('first_frame_mask_options', {'edit_mask_first_frame': 'yes'},
     "edit_mask_first_frame='yes': true or false"),
    ('masked_edit_options', {'edit_mask_path': 'm.png', 'edit_mask_first_frame': 0},
     'edit_mask_first_frame=0: true or false'),
    ('track_options', {'edit_mask_first_frame': True, 'edit_mask_track': 1},
     'edit_mask_track=1: true or false'),
    ('track_options', {'edit_mask_first_frame': True, 'edit_mask_track': True, 'edit_mask_track_median': 'no'},
     "edit_mask_track_median='no': true or false"),
    ('composite_options', {'edit_mask_auto': True, 'edit_mask_composite': 'yes'},
     "edit_mask_composite='yes': true or false"),
    ('composite_options', {'edit_mask_auto': True, 'edit_mask_composite': True, 'edit_mask_match_color': 1},
     'edit_mask_match_color=1: true or false'),
]


def _config(keys):
    return OmegaConf.create({**BASE, **keys})


def test_tables_are_large_enough():
    assert len(ACCEPTED) >= 20 and len(REFUSED) >= 20


@pytest.mark.parametrize("row", ACCEPTED, ids=lambda r: ",".join(k[10:] for k in r[0]) or "none")
def test_accepted(row):
    keys, *views, suffix = row
    for name, want in zip(FUNCS, views):
        got = getattr(cfgmod, name)(_config(keys))
        assert got == want and type(got) is type(want), name
        if want is not None:   # (2 == 2.0: the types are part of what is pinned)
            types = lambda d: {k: type(v) for k, v in (d.items() if isinstance(d, dict) else enumerate(d))}
            assert types(got) == types(want), name
    assert output_suffix(_config(keys), 1) == suffix


@pytest.mark.parametrize("row", REFUSED, ids=lambda r: r[0][:-8] + ":" + ",".join(k[10:] for k in r[1]))
def test_refused(row):
    name, keys, message = row
    with pytest.raises(ValueError) as e:
        getattr(cfgmod, name)(_config(keys))
    assert str(e.value) == message
    with pytest.raises(ValueError):   # (the runner names the directory through the same functions)
        output_suffix(_config(keys), 1)


# ------------------------------------------------------------------------------------------------ the plan behind the five views
@pytest.mark.parametrize("row", ACCEPTED, ids=lambda r: ",".join(k[10:] for k in r[0]) or "none")
def test_plan_agrees_with_the_views_and_names_the_directory(row):
    from anyv2v_amd.masked_edit import MaskedEditPlan, plan_from_config
    keys, masked, first_frame, track, auto, composite, suffix = row
    plan = plan_from_config(_config(keys))
    if masked is None and first_frame is None and auto is None:
        assert plan is None and track is None and composite is None and suffix == S
        return
    shaped = {"grow": masked[1], "feather": masked[2]} if masked is not None else {k: (auto or first_frame)[k] for k in ("grow", "feather")}
    strip = lambda d: None if d is None else {k: v for k, v in d.items() if k not in shaped}
    want = MaskedEditPlan(source="path" if masked is not None else "auto" if auto is not None else "first_frame",
                          path=None if masked is None else masked[0], auto=strip(auto), first_frame=strip(first_frame), track=track,
                          composite=composite, **shaped)
    assert plan == want and type(plan.grow) is int and type(plan.feather) is float
    assert plan.tag() == suffix[len(S):] and suffix.startswith(S + "_mask-")


def test_limits_in_the_messages_are_the_library_constants():
    """The ranges the configuration keys are held to are the ones the pipeline methods and the kernels have: ``_lib``'s constants."""
    from anyv2v_amd import _lib
    limits = {"edit_mask_grow": _lib.MASK_MAX_GROW, "edit_mask_feather": _lib.MASK_MAX_RADIUS // 3, "edit_mask_track_radius": _lib.TRACK_MAX_RADIUS,
              "edit_mask_composite_grow": _lib.COMPOSITE_MAX_GROW, "edit_mask_composite_feather": _lib.COMPOSITE_MAX_RADIUS // 3}
    seen = set()
    for _name, keys, message in REFUSED:
        for key, hi in limits.items():
            if message.startswith(key + "="):
                assert message.endswith(f"0 <= {key} <= {hi}"), message
                seen.add(key)
    assert seen == set(limits)
    # one above each limit is refused, the limit itself is not
    on = {"edit_mask_first_frame": True, "edit_mask_track": True, "edit_mask_composite": True}
    for key, hi in limits.items():
        with pytest.raises(ValueError, match=f"{key}={hi + 1}"):
            cfgmod.masked_edit_options(_config({**on, key: hi + 1}))
        cfgmod.masked_edit_options(_config({**on, key: hi}))
