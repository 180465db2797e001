"""CPU: the scene pipeline under train.py and predict.py (scene_report.run_stages, predict.plan) driven with fakes -- which
``Result:`` blocks a command line prints, under which tags, what every step is asked to hand on, and in which order a
step's lines come.  The expected values are the behaviour of the drivers before there was a runner (five wrappers in
train.py, a ladder in predict.main), read from them; no device is touched."""
import re
from collections import namedtuple

import numpy as np
import pytest
import torch

import predict
import scene_report as sr

Res = namedtuple('Res', 'labels probs conf entropy')
N, K = 12, 3
TRUTH = np.arange(N) % K
JOB = sr.SceneJob((103, 11, 11, 103, 9), None, torch.device('cpu'), 'B2', test_array=np.arange(N), Y_test=TRUTH)
ALL, NONE = dict(probs=True, conf=True, entropy=True), dict(probs=False, conf=False, entropy=False)


class Fakes:
    """a fake first prediction, fake stage calls and a fake score: each records what it was asked for"""

    def __init__(self):
        self.wants, self.scored = [], []

    def result(self, name, want):
        self.wants.append((name, dict(want)))
        return Res(torch.from_numpy(TRUTH.copy()), torch.full((N, K), 1.0 / K) if want['probs'] else None,
                   torch.ones(N) if want['conf'] else None, torch.zeros(N) if want['entropy'] else None)

    def first(self, tag, timing='first time == %.3f s (%d networks)'):
        return (lambda models, cube, spectra, want: self.result('first', want), timing, tag)

    def stage(self, suffix, timing=None):
        return (timing or 'stage' + suffix + ' time == %.3f s', suffix, lambda res, cube, want: self.result(suffix, want))

    def score(self, tag, res):
        assert res.probs is not None            # (a score reads the probabilities of the block it stands behind)
        self.scored.append(tag)
        print('Reliability%s: fake' % tag)


def blocks(text):
    return re.findall(r'^ OA(\w*)=', text, re.M)


# the command line behind `--ckpt x --synthetic B2`: evaluate_whole first, the blocks the runner prints, the Reliability
# tags, where the label map comes from
TABLE = [
    ('--net 0', True, [], [], 'evaluate'),
    ('--net both', True, [], [], 'stacked'),
    ('--net 1 --proba p', True, [], [], 'evaluate'),
    ('--net ensemble', False, ['_ens'], [], 'last'),
    ('--net ensemble --tta 2', False, ['_tta'], [], 'last'),
    ('--net 1 --tta 2 --tta_spatial d4', False, ['_tta_d4'], [], 'last'),
    ('--net ensemble --smooth 2', False, ['_ens', '_ens_smooth'], [], 'last'),
    ('--net 1 --smooth 2', True, ['1_smooth'], [], 'last'),
    ('--net ensemble --superpixel 4', False, ['_ens', '_ens_sp'], [], 'last'),
    ('--net 0 --superpixel 4 --reliability', True, ['_sp'], ['', '_sp'], 'last'),
    ('--net ensemble --smooth 2 --superpixel 4 --temperature 2 --reliability', False,
     ['_ens', '_ens_smooth', '_ens_smooth_sp', '_ens_smooth_sp_T'], ['_ens', '_ens_smooth', '_ens_smooth_sp', '_ens_smooth_sp_T'], 'last'),
    ('--net 0 --reliability', True, [], [''], 'evaluate'),
    ('--net 0 --temperature 2', True, ['_T'], [], 'last'),
    ('--net 0 --temperature fit --reliability', True, ['_T'], ['', '_T'], 'last'),
    ('--net ensemble --tta 2 --smooth 2 --temperature fit --reliability', False,
     ['_tta', '_tta_smooth', '_tta_smooth_T'], ['_tta', '_tta_smooth', '_tta_smooth_T'], 'last'),
]


@pytest.mark.parametrize('line,evaluate,printed,scored,labels', TABLE, ids=[row[0] for row in TABLE])
def test_predict_plans_what_the_ladder_did(line, evaluate, printed, scored, labels, capsys):
    args = predict.build_parser().parse_args(['--ckpt', 'x', '--synthetic', 'B2', *line.split()])
    predict.check_args(args)
    todo = predict.plan(args, True)
    assert todo.evaluate is evaluate and todo.labels == labels
    fit, score = predict.calibration(args, todo, JOB)
    assert (score is not None) == args.reliability
    if 'fit' in line:                                       # a seeded half fits, the Reliability lines say they are the rest's
        assert len(fit[0]) == len(fit[1]) == N // 2
        assert score is None or score.note == ' (held-out n=%d)' % (N - N // 2)
    else:
        assert fit is None and (score is None or score.note == '')
    fakes, job = Fakes(), JOB
    if todo.first_block is None:
        assert not printed and not scored
        return
    if todo.first_block == sr.SILENT and not todo.stages:    # (as predict.main: only --proba etc. read this prediction)
        job = job._replace(test_array=None)
    first = sr.ensemble_first(todo.tag) if todo.tta is None else sr.tta_first(todo.tta)
    assert first.tag == todo.tag
    # the real stages of this command line -- their timing lines and suffixes -- around fake calls
    stages = [fakes.stage(suffix, timing) for timing, suffix, *_ in predict.build_stages(todo.stages, job, args, fit)]
    want = dict(probs=bool(args.proba), conf=bool(args.confidence), entropy=bool(args.entropy))
    sr.run_stages(fakes.first(first.tag, first.timing), stages, None, None, [None] * 2, job, first_block=todo.first_block,
                  want=want, score=fakes.score if score is not None else None)
    assert blocks(capsys.readouterr().out) == printed and fakes.scored == scored


def test_plan_needs_the_test_pixels_for_reliability_and_fit():
    for flags in (['--reliability'], ['--temperature', 'fit']):
        args = predict.build_parser().parse_args(['--ckpt', 'x', '--synthetic', 'B2', *flags])
        with pytest.raises(SystemExit):
            predict.plan(args, False)
    assert predict.plan(predict.build_parser().parse_args(['--ckpt', 'x', '--temperature', '2']), False).stages == (('temper', 2.0),)


def test_tta_of_the_plan_takes_the_checkpoints_noise_by_default():
    p = predict.build_parser()
    assert predict.plan(p.parse_args(['--ckpt', 'x', '--tta', '3']), True, noise=0.25).tta.sigma == 0.25
    tta = predict.plan(p.parse_args(['--ckpt', 'x', '--tta', '3', '--tta_noise', '0', '--tta_no_clean', '--tta_seed', '7']), True, 0.25).tta
    assert (tta.views, tta.sigma, tta.seed, tta.clean, tta.spatial) == (3, 0.0, 7, False, 'none')


@pytest.mark.parametrize('scored', [False, True])
def test_every_step_but_the_last_hands_on_probabilities_only(scored, capsys):
    fakes = Fakes()
    stages = [fakes.stage(s) for s in (sr.SMOOTH_TAG, sr.SP_TAG, sr.TEMPER_TAG)]
    want = dict(conf=True)
    out = sr.run_stages(fakes.first('_x'), stages, None, None, [None], JOB, want=want, score=fakes.score if scored else None)
    assert [name for name, _ in fakes.wants] == ['first', sr.SMOOTH_TAG, sr.SP_TAG, sr.TEMPER_TAG]
    assert all(w == dict(NONE, probs=True) for _, w in fakes.wants[:-1])
    assert fakes.wants[-1][1] == dict(NONE, conf=True, probs=scored)       # the user's wishes, plus what a score reads
    assert sorted(out) == (['conf', 'labels', 'probs'] if scored else ['conf', 'labels'])     # what was not produced is absent
    assert out['labels'].dtype == np.int64 and isinstance(out['conf'], np.ndarray)
    assert want == dict(conf=True)                          # (the caller's dict is left as it is)
    capsys.readouterr()


def test_without_stages_the_first_prediction_takes_the_users_wishes():
    for want in (ALL, NONE, dict(NONE, entropy=True)):
        fakes = Fakes()
        out = sr.run_stages(fakes.first('_x'), [], None, None, [None], JOB, want=want)
        assert fakes.wants == [('first', want)] and sorted(out) == sorted(['labels'] + [k for k, v in want.items() if v])
    fakes = Fakes()
    sr.run_stages(fakes.first('_x'), [], None, None, [None], JOB, score=fakes.score)
    assert fakes.wants == [('first', dict(NONE, probs=True))] and fakes.scored == ['_x']


def test_the_runner_alone_composes_the_tags(capsys):
    """a made-up fourth stage behind the three real ones: its block carries all four suffixes, so no tag is put together
    anywhere but in the runner"""
    fakes = Fakes()
    real = [sr.smooth_stage(predict.smooth_of(predict.build_parser().parse_args(['--ckpt', 'x', '--smooth', '2']))),
            sr.superpixel_stage(predict.superpixel_of(predict.build_parser().parse_args(['--ckpt', 'x', '--superpixel', '4'])), JOB),
            sr.temper_stage(2.0)]
    assert [stage.suffix for stage in real] == ['_smooth', '_sp', '_T']
    stages = [fakes.stage(stage.suffix, stage.timing) for stage in real] + [fakes.stage('_made_up')]
    sr.run_stages(fakes.first('_base'), stages, None, None, [None], JOB, score=fakes.score)
    tags = ['_base', '_base_smooth', '_base_smooth_sp', '_base_smooth_sp_T', '_base_smooth_sp_T_made_up']
    assert blocks(capsys.readouterr().out) == tags and fakes.scored == tags


@pytest.mark.parametrize('mode,printed,scored', [(sr.PRINT, ['_x', '_x_s'], ['_x', '_x_s']), (sr.SCORE, ['_x_s'], ['_x', '_x_s']),
                                                 (sr.SILENT, ['_x_s'], ['_x_s'])])
def test_the_three_modes_of_the_first_block(mode, printed, scored, capsys):
    fakes = Fakes()
    sr.run_stages(fakes.first('_x'), [fakes.stage('_s')], None, None, [None], JOB, first_block=mode, score=fakes.score)
    assert blocks(capsys.readouterr().out) == printed and fakes.scored == scored
    # without the test pixels no block is printed at all
    sr.run_stages(fakes.first('_x'), [fakes.stage('_s')], None, None, [None], JOB._replace(test_array=None), first_block=mode)
    assert blocks(capsys.readouterr().out) == []


def test_the_order_of_a_steps_lines(capsys):
    fakes = Fakes()
    sr.run_stages(fakes.first('_x'), [fakes.stage('_s')], None, None, [None] * 3, JOB, score=fakes.score)
    lines = [line.split('=')[0].split(':')[0].strip() for line in capsys.readouterr().out.splitlines()]
    assert lines == ['first time', 'Result', 'OA_x', 'producerA_x', 'AA_x', 'Reliability_x',
                     'stage_s time', 'Result', 'OA_x_s', 'producerA_x_s', 'AA_x_s', 'Reliability_x_s']


def test_the_first_timing_line_counts_the_networks(capsys):
    sr.run_stages(Fakes().first('_x'), [], None, None, [None] * 3, JOB._replace(test_array=None))
    assert re.fullmatch(r'first time == \d+\.\d{3} s \(3 networks\)\n', capsys.readouterr().out)


def test_who_asks_for_the_cube_is_the_last_stage_that_needs_it():
    """run_scene's refusal names the superpixel vote, else the smoothing, else the first prediction (a window shape the cube-fed
    forward does not take: refused before any network is built)"""
    job = JOB._replace(shape=(103, 20, 20, 103, 9))
    p = predict.build_parser()
    smooth = sr.smooth_stage(predict.smooth_of(p.parse_args(['--ckpt', 'x', '--smooth', '2'])))
    sp = sr.superpixel_stage(predict.superpixel_of(p.parse_args(['--ckpt', 'x', '--superpixel', '4'])), job)
    from cmlpl_amd.tta import TTA
    for first, stages, noun in ((sr.ensemble_first(), [], 'the ensemble'), (sr.tta_first(TTA(2, 0.5)), [], 'test-time augmentation'),
                                (sr.tta_first(TTA(2, 0.5)), [smooth, sr.temper_stage(2.0)], 'spatial smoothing'),
                                (sr.ensemble_first(), [smooth, sp, sr.temper_stage(2.0)], 'the superpixel vote')):
        with pytest.raises(SystemExit) as e:
            sr.run_scene(job, [], first, stages)
        assert str(e.value).startswith(noun + ' needs the scene cube')
