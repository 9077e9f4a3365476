"""Expected goals on the device: shot rows, fit, rate and score.

The reference's ``public-notebooks/EXTRA-build-expected-goals-model.ipynb`` picks the shot rows
of every game's feature frame (``ai.type_name.str.contains("shot")``, ``Xi[shot_idx]``), keeps
46 feature columns, fits a classifier on ``result_success_a0`` and scores it with AUROC, Brier
score and log loss.  Here the features stay in HBM: the shot rows are gathered out of the
bitmap-form feature blocks by ``ops.select_rows`` (``sa_select_rows``) into a compact table a
few per cent the size of the full one, and the device learner (:mod:`socceraction_amd.boost`),
the tree predictor and the score kernels run on that table.  Only the shots ever cross the link.

The notebook fits two models on the shot table, and both are offered: its ``XGBClassifier()``
(``learner='device'``) and its ``LogisticRegression()`` (``learner='logistic'``,
:mod:`socceraction_amd.linear`).  The notebook's own lbfgs fit of the latter stops at the
iteration limit, 0.03 - 0.06 in probability away from the optimum, so it is no reference result;
the optimum itself is one -- the objective is strictly convex -- and the device fit reaches it by
Newton's method on integer sums, bit-identical from run to run and for any row order.
"""
from __future__ import annotations

import math
import re
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import pandas as pd
import torch
from sklearn.exceptions import NotFittedError

from . import ops
from .batch import ActionBatch
from .spadl import config as spadlcfg
from .vaep import features as fs

# the notebook's cell 7
XFNS = [fs.actiontype_onehot, fs.bodypart_onehot, fs.startlocation, fs.movement, fs.space_delta,
        fs.startpolar, fs.team]
NB_PREV_ACTIONS = 2
# what XGBClassifier() means there: 100 trees of depth 6 at learning rate 0.3
TREE_PARAMS = dict(n_estimators=100, max_depth=6, learning_rate=0.3)
SHOT_TYPES = tuple(i for i, t in enumerate(spadlcfg.actiontypes) if 'shot' in t)
# what LogisticRegression() means there: C = 1 with an intercept (solved to the optimum here)
LINEAR_PARAMS = dict(C=1.0, fit_intercept=True, tol=1e-10, max_iter=100)
SUCCESS = spadlcfg.results.index('success')
_LEAKS = ('dx_a0', 'dy_a0', 'movement_a0')  # a shot's own movement gives its result away


def feature_names(xfns: Optional[Sequence[Any]] = None, nb_prev_actions: int = NB_PREV_ACTIONS) -> List[str]:
    """The model's features (the notebook's cell 7): ``feature_column_names`` without the shot's
    own action type (``type_*_a0``: it was selected on) and without ``dx_a0``, ``dy_a0`` and
    ``movement_a0``, which leak the result.  46 names for the defaults."""
    names = fs.feature_column_names(XFNS if xfns is None else list(xfns), nb_prev_actions)
    return [c for c in names if not re.match('type_[a-z_]+_a0', c) and c not in _LEAKS]


def shot_rows(batch: ActionBatch) -> torch.Tensor:
    """The row numbers of ``batch``'s shots (:data:`SHOT_TYPES`), ascending, int64 on the device."""
    t = batch.cols['type_id'][:batch.n]
    mask = torch.zeros_like(t, dtype=torch.bool)
    for s in SHOT_TYPES:
        mask |= t == s
    return torch.nonzero(mask).reshape(-1)


def shot_labels(batch: ActionBatch, rows: torch.Tensor) -> torch.Tensor:
    """``result_id == success`` of the listed rows as a uint8 device column: the notebook's
    ``result_success_a0`` on those rows."""
    return (batch.cols['result_id'][:batch.n][rows] == SUCCESS).to(torch.uint8).contiguous()


def _known_xfns(xfns: Sequence[Any]) -> List[str]:
    known = [fs.xfn_name(f, False) for f in xfns]
    if any(k is None for k in known):
        raise ValueError('expected goals on the device needs built-in feature transformers')
    return known


def _game_batch(games: pd.DataFrame, actions: pd.DataFrame) -> ActionBatch:
    home_of = games.set_index('game_id')['home_team_id']
    return ActionBatch.from_frame(actions, home_team_id=home_of, segments='game')


def _shot_blocks(ab: ActionBatch, known: Sequence[str], k: int):
    """``(shot rows, their compact feature blocks)``: features, then ``select_rows``."""
    fb = ops.features(ab, known, k, bool_bits=True)
    rows = shot_rows(ab)
    return rows, ops.select_rows(fb, rows)


def get_shots(games: pd.DataFrame, actions: pd.DataFrame, xfns: Optional[Sequence[Any]] = None,
              nb_prev_actions: int = 3) -> pd.DataFrame:
    """The notebook's ``get_shots`` without the stores: the feature frame (default: VAEP's
    transformers, as its ``features.h5`` holds them) of the shot rows only, indexed by their
    positions in ``actions``.  The features of every action are computed on the device, the shot
    rows are gathered there and only they are copied to the host."""
    from .vaep.base import xfns_default
    known = _known_xfns(xfns_default if xfns is None else xfns)
    rows, compact = _shot_blocks(_game_batch(games, actions), known, nb_prev_actions)
    return compact.to_frame(index=pd.Index(rows.cpu().numpy()))


class _LinearPredictor:
    """A fitted linear model behind the tree predictor's ``predict_blocks``: float32 P(class 1)
    of every row of bitmap-form feature blocks."""

    def __init__(self, model) -> None:
        self.model = model

    def predict_blocks(self, blocks) -> torch.Tensor:
        return self.model.predict_blocks(blocks, dtype=torch.float32)


def _predictor(model):
    """The one seam between the two model kinds: an object whose ``predict_blocks(blocks)`` gives
    float32 probabilities on the device."""
    from .linear import DeviceLogisticRegression
    if isinstance(model, DeviceLogisticRegression):
        return _LinearPredictor(model)
    from .trees import TreeEnsemble
    return TreeEnsemble.from_model(model)


class ExpectedGoals:
    """An expected-goals model of the notebook's kind, fitted, applied and scored on the device.

    Parameters
    ----------
    xfns : list
        Feature transformers (default :data:`XFNS`, the notebook's); built-in ones only.
    nb_prev_actions : int, default=2
        Number of previous actions in a game state.
    columns : list of str
        The model's features, in model order (default :func:`feature_names` of the above).
    """

    def __init__(self, xfns: Optional[List[Any]] = None, nb_prev_actions: int = NB_PREV_ACTIONS,
                 columns: Optional[Sequence[str]] = None) -> None:
        self.xfns = XFNS if xfns is None else xfns
        self.nb_prev_actions = nb_prev_actions
        self.columns = None if columns is None else [str(c) for c in columns]
        self.model_ = None
        self._predictor = None
        self.device_eval_: Optional[Dict[str, float]] = None

    def _columns(self) -> List[str]:
        return feature_names(self.xfns, self.nb_prev_actions) if self.columns is None else self.columns

    # ---------------------------------------------------------------- fitting
    def fit_batch(self, games: pd.DataFrame, actions: pd.DataFrame, learner: str = 'device',
                  tree_params: Optional[Dict[str, Any]] = None, val_size: float = 0.0,
                  early_stopping_rounds: Optional[int] = None, eval_metric: str = 'auc',
                  sample_weight=None, linear_params: Optional[Dict[str, Any]] = None) -> 'ExpectedGoals':
        """Fit the model on the shots of many games (contiguous per game): one ``ActionBatch``,
        the features as bitmaps plus numeric blocks, the shot rows gathered into a compact table
        (``ops.select_rows``), that table binned on the model's columns and the learner fitted
        on all of it -- no row mask: the histogram kernels stream the shots, not the actions.

        ``tree_params``: the device learner's, over :data:`TREE_PARAMS`.  ``val_size``: the share
        of the SHOTS (a random split, as ``VAEP.fit_batch`` splits its rows) held out and scored
        once after training into ``self.device_eval_``; the training shots are then a mask over
        the compact table.  ``early_stopping_rounds`` (needs ``val_size > 0``) and
        ``eval_metric``: as in ``VAEP.fit_batch``.  ``sample_weight``: one weight per row of
        ``actions``; the shots' are gathered.  With ``subsample`` a round's row sample is keyed by
        ``fm(game_id) + action_id`` of the shot.

        ``learner='logistic'``: the notebook's other model, a
        :class:`~socceraction_amd.linear.DeviceLogisticRegression` (``linear_params`` over
        :data:`LINEAR_PARAMS`) on the same compact table and columns, the training shots again a
        mask when ``val_size`` holds some out.  It has no rounds to stop early and takes no
        weights: ``early_stopping_rounds``, ``sample_weight`` and ``tree_params`` are a ``ValueError``
        (``eval_metric`` names what early stopping watches and is not looked at)."""
        from . import boost
        from .vaep.base import VAEP
        if learner == 'logistic':
            if tree_params is not None:
                raise ValueError('tree_params go with learner=\'device\'')
            return self._fit_logistic(games, actions, linear_params, val_size, early_stopping_rounds, sample_weight)
        if learner != 'device':
            raise ValueError(f'A {learner} learner is not supported by fit_batch')
        if linear_params is not None:
            raise ValueError('linear_params go with learner=\'logistic\'')
        params = boost.check_params({**TREE_PARAMS, **dict(tree_params or {})})  # before any device call
        stop = VAEP._device_stop_params(early_stopping_rounds, eval_metric, val_size > 0)
        weight = sample_weight
        if weight is not None:
            weight, _ = boost.check_weights(weight, len(actions), None, params['scale_pos_weight'])
        sampled = boost.row_threshold(params['subsample']) != boost.THR_ALL
        if sampled and not {'game_id', 'action_id'} <= set(actions.columns):
            raise ValueError('subsample needs the game_id and action_id columns (they key the row sample)')
        known = _known_xfns(self.xfns)
        columns = self._columns()
        ab, rows, y, compact, train, val = self._shot_table(games, actions, known, val_size)
        data = boost.bin_blocks(compact, rows=train, columns=columns)
        host_rows = rows.cpu().numpy() if (sampled or weight is not None) else None
        keys = boost.row_keys(actions['game_id'].to_numpy()[host_rows], actions['action_id'].to_numpy()[host_rows],
                              ab.device) if sampled else None
        if weight is not None:
            weight = boost.weights_to_device(weight[host_rows], ab.device)
        eval_rows = val if stop['early_stopping_rounds'] is not None else None
        clf = boost.make_classifier(params, **stop).fit_binned(data, y, train, eval_rows, weight, keys)
        return self._fitted_model(clf, columns, compact, y, val)

    def _shot_table(self, games: pd.DataFrame, actions: pd.DataFrame, known: Sequence[str], val_size: float):
        """``(batch, shot rows, labels, compact blocks, training rows, held-out rows)``: what either
        learner is fitted on.  The row lists index the compact table (``None`` without a split)."""
        ab = _game_batch(games, actions)
        rows = shot_rows(ab)
        m = int(rows.numel())
        if m == 0:
            raise ValueError('there are no shots among the actions')
        y = shot_labels(ab, rows)
        n_pos = int(y.sum())
        if n_pos == 0 or n_pos == m:
            raise ValueError('Only one class present among the shots.')
        fb = ops.features(ab, known, self.nb_prev_actions, bool_bits=True)
        compact = ops.select_rows(fb, rows)
        train = val = None
        if val_size > 0:
            idx = np.random.permutation(m)
            cut = math.floor(m * (1 - val_size))
            train = torch.from_numpy(np.sort(idx[:cut])).to(ab.device)
            val = torch.from_numpy(np.sort(idx[cut + 1:])).to(ab.device)
        return ab, rows, y, compact, train, val

    def _fitted_model(self, model, columns: Sequence[str], compact, y, val) -> 'ExpectedGoals':
        """Keep ``model``; with held-out shots, score it on them once into ``device_eval_``."""
        from . import metrics
        self.device_eval_ = None
        if val is not None and val.numel():
            p = _predictor(model).predict_blocks(compact)
            self.device_eval_ = metrics.binary_scores(y[val].contiguous(), p[val].contiguous())
        self.model_ = model
        self.feature_names_in_ = list(columns)
        self._predictor = None
        return self

    def _fit_logistic(self, games, actions, linear_params, val_size, early_stopping_rounds, sample_weight):
        from . import linear
        if early_stopping_rounds is not None:
            raise ValueError('early_stopping_rounds needs a learner that trains in rounds: the logistic learner '
                             'solves to the optimum')
        if sample_weight is not None:
            raise ValueError('the logistic learner takes no sample weights')
        params = {**LINEAR_PARAMS, **dict(linear_params or {})}
        unknown = sorted(set(params) - set(LINEAR_PARAMS))
        if unknown:
            raise ValueError(f'unknown linear_params: {unknown}')
        linear.check_params(params['C'], params['tol'], params['max_iter'])  # before any device call
        known = _known_xfns(self.xfns)
        columns = self._columns()
        _, _, y, compact, train, val = self._shot_table(games, actions, known, val_size)
        model = linear.DeviceLogisticRegression(**params).fit_blocks(compact, y, rows=train, columns=columns)
        return self._fitted_model(model, columns, compact, y, val)

    def _fitted(self):
        if self.model_ is None:
            raise NotFittedError()
        if self._predictor is None:
            self._predictor = _predictor(self.model_)
        return self._predictor

    def to_xgboost_json(self) -> dict:
        """The fitted classifier as an xgboost-1.6-shaped JSON model (the tree learner's only)."""
        self._fitted()
        if not hasattr(self.model_, 'to_xgboost_json'):
            raise ValueError('a logistic model has no xgboost form: its parameters are model_.coef_ and '
                             'model_.intercept_')
        return self.model_.to_xgboost_json()

    # ---------------------------------------------------------------- rating
    def _rate(self, ab: ActionBatch):
        """``(shot rows, their labels, their xG)``, all on the device."""
        predictor = self._fitted()
        rows, compact = _shot_blocks(ab, _known_xfns(self.xfns), self.nb_prev_actions)
        if rows.numel() == 0:
            return rows, shot_labels(ab, rows), torch.zeros(0, dtype=torch.float32, device=ab.device)
        return rows, shot_labels(ab, rows), predictor.predict_blocks(compact)

    @staticmethod
    def _frame(actions: pd.DataFrame, rows: torch.Tensor, p: torch.Tensor) -> pd.DataFrame:
        return pd.DataFrame({'xg': p.cpu().numpy().astype(np.float32, copy=False)},
                            index=actions.index[rows.cpu().numpy()])

    def rate_batch(self, games: pd.DataFrame, actions: pd.DataFrame) -> pd.DataFrame:
        """The expected-goals value of every shot of many games (contiguous per game): one
        float32 column ``xg``, indexed by the shots' index in ``actions``.  Features, the shot
        rows' gather and the tree walk over the compact blocks all run on the device; one value
        per shot is copied back."""
        self._fitted()
        rows, _, p = self._rate(_game_batch(games, actions))
        return self._frame(actions, rows, p)

    def rate(self, game: pd.Series, game_actions: pd.DataFrame) -> pd.DataFrame:
        """:meth:`rate_batch` of one game."""
        self._fitted()
        rows, _, p = self._rate(ActionBatch.from_frame(game_actions, home_team_id=game.home_team_id))
        return self._frame(game_actions, rows, p)

    def score_batch(self, games: pd.DataFrame, actions: pd.DataFrame) -> Dict[str, float]:
        """:func:`socceraction_amd.metrics.binary_scores` of the shots' labels against their
        ``xg``, on the device: Brier score, log loss, AUROC, ``n``, ``n_pos`` and the Brier score
        and log loss of the base-rate prediction (``*_baseline``).  The base rate is the SCORED
        set's own; the notebook's last cell predicts the TRAINING set's rate instead, so its
        baseline figures differ from these whenever the two rates do."""
        from . import metrics
        self._fitted()
        rows, y, p = self._rate(_game_batch(games, actions))
        if rows.numel() == 0:
            raise ValueError('there are no shots among the actions')
        return metrics.binary_scores(y, p.contiguous())
