"""`Logger` of the reference's Link_prediction_model/logger.py: one list of evaluation results per run, the reference's statistics and their text.
A result is a tuple whose entry 0 selects the evaluation point ("valid") and whose entry 1 is reported there ("test"); both are printed as
percentages.  last_best takes the LAST evaluation that reaches the run's maximum, otherwise the first.  The numbers pass through float32 tensors
as in the reference, so the printed digits are its digits."""
import sys

import torch


def _best_point(valid, last_best):
    """Index of the maximum of a 1-D tensor: its first occurrence, or its last."""
    if not last_best:
        return int(valid.argmax().item())
    return valid.numel() - 1 - int(valid.flip(dims=[0]).argmax().item())


class Logger(object):
    def __init__(self, runs, info=None):
        self.info = info
        self.results = [[] for _ in range(runs)]

    def add_result(self, run, result):
        assert 0 <= run < len(self.results)
        self.results[run].append(result)

    def best_of_run(self, run, last_best=False):
        """(highest valid, evaluation point (0-based), test at that point) of one run, in percent."""
        table = 100 * torch.tensor(self.results[run])
        at = _best_point(table[:, 0], last_best)
        return table[:, 0].max(), at, table[at, 1]

    def print_statistics(self, run=None, f=sys.stdout, last_best=False):
        if run is not None:
            valid, at, test = self.best_of_run(run, last_best)
            lines = [f'Run {run + 1:02d}:', f'Highest Valid: {valid:.2f}', f'Highest Eval Point: {at + 1}', f'   Final Test: {test:.2f}']
        else:
            best = torch.tensor([[v.item(), t.item()] for v, _, t in (self.best_of_run(r, last_best) for r in range(len(self.results)))])
            lines = ['All runs:', f'Highest Valid: {best[:, 0].mean():.2f}  {best[:, 0].std():.2f}',
                     f'   Final Test: {best[:, 1].mean():.2f}  {best[:, 1].std():.2f}']
        for line in lines:
            print(line, file=f)
