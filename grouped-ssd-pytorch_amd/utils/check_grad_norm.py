"""``check_grad_norm(model)`` of the reference drivers (``from utils.check_grad_norm import check_grad_norm``, called between
``loss.backward()`` and the clip on every iteration) on ``gssd.grad_stats``: two launches for all parameters and ONE read of the total,
where a norm per parameter costs a launch and a read each."""
from gssd.grad_stats import grad_stats


def check_grad_norm(model):
    """The 2-norm of all gradients of ``model`` as a Python float.  Every parameter must have a gradient: one whose ``.grad`` is None
    raises AttributeError naming it.  For the per-parameter table behind the number, or to log without a read per step, see
    ``gssd.optim.grad_stats`` / ``GradMonitor``."""
    stats = grad_stats(model, params=False)
    if stats.without_grad:
        raise AttributeError(f'check_grad_norm: parameter {stats.without_grad[0]!r} has no gradient (.grad is None)'
                             + (f', nor have {len(stats.without_grad) - 1} more' if len(stats.without_grad) > 1 else ''))
    return stats.total_norm.item()
