"""Loss reporting on the host (no GPU): args.log_losses in Coach.learn and main.py.

The key is opt-in: without it Coach.learn never calls evaluate; with it evaluate runs twice per
iteration and one JSON line per iteration goes to <checkpoint>/losses.jsonl, while the examples,
the arena results and the state of both host RNGs (random, np.random) after the run are those of
the run without the key -- so the shuffles and draws are the same ones."""
import json
import os
import pickle
import random
from types import SimpleNamespace

import numpy as np
import pytest

from test_native_mcts import HashNet
from test_selfplay import _norm_gnn, _norm_std


class Args(SimpleNamespace):
    def __getitem__(self, k):
        return getattr(self, k)

    def get(self, k, default=None):
        return getattr(self, k, default)


class RecordingNet(HashNet):
    """HashNet behind the wrappers' surface: train() moves the salt (the 'weights'), checkpoints
    carry it, evaluate() returns metrics that depend on it; every call is recorded."""

    def __init__(self, game, args):
        super().__init__(game.getActionSize(), 11)
        self.calls = []

    def train(self, examples, gnn_examples=None):
        self.calls.append(("train", len(examples), len(gnn_examples or [])))
        self.salt += 1
        self.last_train_losses = [{"epoch": 0, "loss_pi": 2.0, "loss_v": 1.0, "loss": 3.0},
                                  {"epoch": 1, "loss_pi": 1.5, "loss_v": 0.5, "loss": 2.0}]

    def evaluate(self, examples, gnn_examples=None, chunk=4096):
        self.calls.append(("evaluate", len(examples), len(gnn_examples or []), self.salt))
        out = {"loss_pi": 1.0 / self.salt, "loss_v": 0.25, "loss": 1.0 / self.salt + 0.25,
               "top1": 0.5, "entropy": 1.0, "target_entropy": 0.5, "n": len(examples)}
        if gnn_examples is not None:
            for prefix in ("gnn_", "std_on_gnn_"):
                out.update({prefix + k: v for k, v in list(out.items())[:7]})
                out[prefix + "n"] = len(gnn_examples)
        return out

    def save_checkpoint(self, folder, filename):
        os.makedirs(folder, exist_ok=True)
        with open(os.path.join(folder, filename), "wb") as f:
            pickle.dump(self.salt, f)

    def load_checkpoint(self, folder, filename):
        with open(os.path.join(folder, filename), "rb") as f:
            self.salt = pickle.load(f)


def _learn(tmp_path, monkeypatch, name, engine, use_gnn, **extra):
    import Coach as C
    from tictactoe.TicTacToeGame import TicTacToeGame
    game = TicTacToeGame(3)
    args = Args(numIters=2, numEps=2, numMCTSSims=4, cpuct=1.0, tempThreshold=3, use_gnn=use_gnn,
                expand_by=1, arenaCompare=2, updateThreshold=0.5, maxlenOfQueue=1000,
                numItersForTrainExamplesHistory=2, checkpoint=str(tmp_path / name),
                selfplay_engine=engine, parallel_games=1, **extra)
    arena = []
    orig = C.Arena.playGames
    monkeypatch.setattr(C.Arena, "playGames",
                        lambda self, *a, **k: (arena.append(orig(self, *a, **k)), arena[-1])[1])
    random.seed(5)
    np.random.seed(6)
    coach = C.Coach(game, RecordingNet(game, args), args)
    coach.learn()
    monkeypatch.undo()
    hist = [(_norm_std(std), _norm_gnn(gnn)) for std, gnn in coach.trainExamplesHistory]
    files = sorted(os.listdir(args.checkpoint)) if os.path.isdir(args.checkpoint) else []
    return dict(coach=coach, hist=hist, arena=arena, files=files, folder=args.checkpoint,
                rng=(random.getstate(), np.random.get_state()[1].tolist(),
                     np.random.get_state()[2]))


@pytest.mark.parametrize("use_gnn", [False, True])
@pytest.mark.parametrize("engine", ["python", "native"])
def test_log_losses_changes_nothing_but_the_report(tmp_path, monkeypatch, caplog, engine, use_gnn):
    """Fails without the feature: Coach.learn never calls evaluate and writes no losses.jsonl."""
    import logging
    off = _learn(tmp_path, monkeypatch, "off", engine, use_gnn)
    absent_false = _learn(tmp_path, monkeypatch, "false", engine, use_gnn, log_losses=False)
    with caplog.at_level(logging.INFO, logger="Coach"):
        on = _learn(tmp_path, monkeypatch, "on", engine, use_gnn, log_losses=True)
    lines = [r.getMessage() for r in caplog.records if "LOSS" in r.getMessage()]
    for run in (off, absent_false):
        calls = run["coach"].nnet.calls
        assert [c[0] for c in calls] == ["train", "train"]
        assert "losses.jsonl" not in run["files"]
    # the key on: evaluate before and after every train(), on the lists train() gets
    calls = on["coach"].nnet.calls
    assert [c[0] for c in calls] == ["evaluate", "train", "evaluate"] * 2
    for it in range(2):
        ev0, tr, ev1 = calls[3 * it:3 * it + 3]
        assert ev0[1:3] == tr[1:3] == ev1[1:3]
        assert ev1[3] == ev0[3] + 1                       # the second one sees the trained net
        assert (tr[2] > 0) == use_gnn
    assert all(c[0] != "evaluate" for c in on["coach"].pnet.calls)
    # examples, arena results, both host RNG streams, the other files: as without the key
    assert on["hist"] == off["hist"] == absent_false["hist"]
    assert on["arena"] == off["arena"] == absent_false["arena"] and len(on["arena"]) == 2
    assert on["rng"] == off["rng"] == absent_false["rng"]
    assert [f for f in on["files"] if f != "losses.jsonl"] == off["files"]
    for f in off["files"]:
        a = open(os.path.join(off["folder"], f), "rb").read()
        assert a == open(os.path.join(on["folder"], f), "rb").read(), f
    # one well-formed line per iteration
    rows = [json.loads(l) for l in open(os.path.join(on["folder"], "losses.jsonl"))]
    assert [r["iteration"] for r in rows] == [1, 2]
    for r, it in zip(rows, range(2)):
        assert set(r) == {"iteration", "before", "after", "train_epochs"}
        want = {"loss_pi", "loss_v", "loss", "top1", "entropy", "target_entropy", "n"}
        if use_gnn:
            want |= {p + k for p in ("gnn_", "std_on_gnn_") for k in want}
        assert set(r["before"]) == set(r["after"]) == want
        assert r["before"]["n"] == calls[3 * it][1] and r["after"]["loss_pi"] < r["before"]["loss_pi"]
        assert [e["epoch"] for e in r["train_epochs"]] == [0, 1]
    # two lines per iteration and the first / last epoch's training loss
    assert len([l for l in lines if l.startswith("LOSSES iter")]) == 4
    assert len([l for l in lines if l.startswith("TRAIN LOSS iter")]) == 2
    assert "'epoch': 0" in lines[2] and "'epoch': 1" in lines[2]


def test_only_the_writer_rank_reports(tmp_path, monkeypatch):
    import Coach as C
    monkeypatch.setattr(C.Coach, "_is_writer", lambda self: False)
    monkeypatch.setattr(C.Coach, "saveTrainExamples", lambda self, i: None)
    orig_load = RecordingNet.load_checkpoint
    monkeypatch.setattr(RecordingNet, "load_checkpoint",
                        lambda self, folder, filename: None if not os.path.exists(
                            os.path.join(folder, filename)) else orig_load(self, folder, filename))
    run = _learn(tmp_path, monkeypatch, "rank1", "python", True, log_losses=True)
    assert [c[0] for c in run["coach"].nnet.calls] == ["evaluate", "train", "evaluate"] * 2
    assert "losses.jsonl" not in run["files"]


def test_main_carries_log_losses(tmp_path):
    import main
    import yaml
    cfg = tmp_path / "config.yaml"
    doc = {"game": {"board_size": 3}, "training": {"checkpoint_path": str(tmp_path / "ck")}}
    cfg.write_text(yaml.safe_dump(doc))
    base = ["--game", "tictactoe", "--config", str(cfg)]
    assert main.parse(base).log_losses is None
    assert not main.build_args(main.parse(base)).get("log_losses", False)
    assert main.build_args(main.parse(base + ["--log_losses"])).log_losses is True
    doc["training"]["log_losses"] = True
    cfg.write_text(yaml.safe_dump(doc))
    assert main.build_args(main.parse(base)).log_losses is True
    for name in ("connect4", "tictactoe", "frozenlake"):      # the shipped configs name the key, off
        shipped = main.load_config(os.path.join(main.HERE, name, "config.yaml"))
        assert shipped["training"]["log_losses"] is False
    assert "--log_losses" in main.__doc__
