"""ops.options: the one table of training options agrees with the flags, the README and itself."""
import os
import re

import pytest

from distributed_tensorflow_for_dcgan_amd.ops import options as O
from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.utils import flags as F

README = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "README.md")


@pytest.fixture(autouse=True)
def clean_environment(monkeypatch):
    for name in O.ENV_NAMES:
        monkeypatch.delenv(name, raising=False)


def test_every_flag_of_the_table_exists():
    names = {n for n, _, _, _ in F.ALL_FLAGS}
    for g in O.TABLE.values():
        assert len(g.flag_names) == len(g.keywords) == len(g.env) == len(g.conv) == len(g.defaults)
        assert set(g.flag_names) <= names, g.flag_names
        assert set(g.fields) <= set(O.StepOptions._fields)
        assert g.steps is None or g.steps in g.keywords and g.stand_in is not None
    assert [g.steps_flag for g in O.ANNEALED] == ["lr_decay_steps", "instance_noise_steps", "g_topk_steps"]


def test_flag_defaults_are_the_keyword_defaults():
    fl = F.parse_flags([])
    assert O.resolve(int(fl.batch_size), env=False, **O.from_flags(fl)) == O.resolve(int(fl.batch_size), env=False)
    assert O.open_ended(O.from_flags(fl)) == []


def test_every_environment_variable_is_in_the_readme():
    with open(README) as f:
        rows = [line for line in f if line.startswith("| `DCGAN_")]
    documented = set(re.findall(r"`(DCGAN_[A-Z0-9_]+)`", "".join(row.split("|")[1] for row in rows)))
    assert set(O.ENV_NAMES) <= documented, sorted(set(O.ENV_NAMES) - documented)
    assert len(set(O.ENV_NAMES)) == len(O.ENV_NAMES)


# one non-default setting per group: engine keywords, and the record fields they must give
AUG = dict(d_augment="translation,cutout", d_color_augment="brightness")
SETTINGS = {
    "d_steps": (dict(d_steps=3, beta2=0.9, lr_d=4e-4, lr_g=1e-4), dict(d_steps=3, beta2=0.9, lr_d=4e-4, lr_g=1e-4)),
    "lr_sched": (dict(lr_decay="cosine", lr_decay_start=5, lr_decay_steps=100, lr_end=0.1, lr_warmup=7),
                 dict(lr_sched=R.LrSchedule("cosine", 5, 100, 0.1, 7))),
    "noise": (dict(instance_noise=0.2, instance_noise_end=0.05, instance_noise_steps=50),
              dict(noise=R.InstanceNoise(0.2, 0.05, 50))),
    "aug": (dict(d_augment="cutout"), dict(aug=R.DAugment(False, True))),
    "color": (dict(d_color_augment="saturation,contrast"), dict(color=R.DColor(False, True, True))),
    "ada": (dict(AUG, d_augment_p=0.25, ada_target=0.6, ada_interval=2, ada_kimg=100.0),
            dict(ada=R.DAda(0.25, 0.6, 2, 100.0))),
    "topk": (dict(g_topk=0.5, g_topk_steps=30), dict(topk=R.GTopK(0.5, 30))),
    "g_ema_decay": (dict(g_ema_decay=0.999), dict(g_ema_decay=0.999)),
    "gan_loss": (dict(gan_loss="lsgan", label_smooth=0.1), dict(gan_loss="lsgan", label_smooth=0.1)),
    "d_spectral_norm": (dict(d_spectral_norm=True), dict(d_spectral_norm=True)),
}


def test_the_settings_cover_the_table():
    assert list(SETTINGS) == list(O.TABLE)
    for name, (kw, _) in SETTINGS.items():
        assert set(O.TABLE[name].keywords) <= set(kw)


def _spellings(kw):
    """(environment, argv) of the engine keywords `kw`."""
    env, argv = {}, []
    for g in O.TABLE.values():
        for k, f, e in zip(g.keywords, g.flag_names, g.env):
            if k in kw:
                env[e] = "1" if kw[k] is True else str(kw[k])
                argv.append("--%s=%s" % (f, kw[k]))
    return env, argv


@pytest.mark.parametrize("name", list(SETTINGS))
def test_keyword_environment_and_flags_give_one_record(name, monkeypatch):
    kw, expect = SETTINGS[name]
    B = 64  # (the flags' default batch size)
    by_keyword = O.resolve(B, **kw)
    assert by_keyword == O.resolve(B, env=False, **kw) != O.resolve(B)
    assert {k: getattr(by_keyword, k) for k in expect} == expect
    env, argv = _spellings(kw)
    by_flags = O.resolve(B, env=False, **O.from_flags(F.parse_flags(argv)))
    assert by_flags == by_keyword
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert O.resolve(B) == O.resolve(B, **{k: None for k in kw}) == by_keyword
    assert O.resolve(B, env=False) == O.resolve(None, env=False)  # (the environment is not read)
    # an explicit keyword beats the variable: the flags' defaults, given as keywords, undo the environment
    assert O.resolve(B, **O.from_flags(F.parse_flags([]))) == O.resolve(B, env=False)
    g = O.TABLE[name]
    monkeypatch.setenv(g.env[0], "")  # set but empty counts as unset
    assert O.resolve(B) == O.resolve(B, env=False, **{k: v for k, v in kw.items() if k != g.keywords[0]})


def test_the_resolved_record_is_accepted_for_its_group():
    o = O.resolve(8, **{k: v for kw, _ in SETTINGS.values() for k, v in kw.items()})
    again = O.resolve(8, env=False, lr_decay=o.lr_sched, instance_noise=o.noise, d_augment=o.aug,
                      d_color_augment=o.color, d_augment_p=o.ada, g_topk=o.topk, d_steps=o.d_steps, beta2=o.beta2,
                      lr_d=o.lr_d, lr_g=o.lr_g, g_ema_decay=o.g_ema_decay, gan_loss=o.gan_loss,
                      label_smooth=o.label_smooth, d_spectral_norm=o.d_spectral_norm)
    assert again == o


def test_conversion_errors_and_unknown_keywords(monkeypatch):
    monkeypatch.setenv("DCGAN_D_STEPS", "three")
    with pytest.raises(ValueError, match="DCGAN_D_STEPS='three' is not a number"):
        O.resolve(8)
    assert O.resolve(8, d_steps=2).d_steps == 2 and O.resolve(8, env=False).d_steps == 1
    with pytest.raises(TypeError, match="lr_decay_stepz"):
        O.resolve(8, env=False, lr_decay_stepz=3)
    assert O.known(dict(d_steps=2, dtype="bf16")) == dict(d_steps=2)


def test_open_ended_steps_resolve_against_the_total():
    fl = F.parse_flags(["--lr_decay=linear", "--lr_decay_start=10", "--instance_noise=0.1", "--g_topk=0.5"])
    kw = O.from_flags(fl)
    assert [g.steps for g in O.open_ended(kw)] == ["lr_decay_steps", "instance_noise_steps", "g_topk_steps"]
    done = O.from_flags(fl, total_steps=100)
    assert (done["lr_decay_steps"], done["instance_noise_steps"], done["g_topk_steps"]) == (90, 100, 100)
    assert O.open_ended(done) == []
    # sample-only mode never steps: the stand-in totals give any valid length
    assert [g.until_end(kw, None) for g in O.ANNEALED] == [1, 1, 1]
    with pytest.raises(ValueError, match="lr_decay_steps=0 decays until the end of training"):
        O.from_flags(fl, total_steps=10)
