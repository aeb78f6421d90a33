"""SimpleGA (the solver ETGRL uses: train.py:288-295, pretrain.py) with the population kept as a
torch tensor on any device, so ask -> Opt_with_points -> rollout -> tell never leaves the GPU.

Mirrors alg/es.py:214-326 (estool's SimpleGA): same constructor arguments, ask()/tell()/result()/
reset()/get_best_param()/current_param(), same elite selection, mating, sigma decay and L2 weight
decay (alg/es.py:29-31).  Random draws come from a torch.Generator; `ask(draws=...)` accepts the
three draw arrays explicitly, which is how the golden test replays the reference's numpy stream.

PEPG, OpenES and SimpleES (alg/es.py:446-619, 328-444, 145-211) follow below in the same conventions: they build their update
from every return of the generation, which is what a population of thousands wants (SimpleGA keeps one return in ten).
make_solver(alg, ...) reproduces the five settings blocks of model/Dynamic_parallel_model.py:102-149.  CMAES is not provided:
it wraps the `cma` package, which this project does not depend on.
"""
import math

import torch


class SimpleGA:
    def __init__(self, num_params, sigma_init=0.1, sigma_decay=0.999, sigma_limit=0.01, popsize=256,
                 elite_ratio=0.1, forget_best=False, weight_decay=0.01, param=None, device="cpu", seed=0,
                 dtype=torch.float64):
        self.num_params, self.popsize = int(num_params), int(popsize)
        self.sigma_init, self.sigma_decay, self.sigma_limit = sigma_init, sigma_decay, sigma_limit
        self.elite_ratio = elite_ratio
        self.elite_popsize = int(self.popsize * self.elite_ratio)
        self.sigma = self.sigma_init
        self.device, self.dtype = torch.device(device), dtype
        self.elite_params = torch.zeros(self.elite_popsize, self.num_params, dtype=dtype, device=self.device)
        self.elite_rewards = torch.zeros(self.elite_popsize, dtype=dtype, device=self.device)
        self.best_param = torch.zeros(self.num_params, dtype=dtype, device=self.device) if param is None else \
            torch.as_tensor(param, dtype=dtype, device=self.device).clone()
        self.curr_best_param = self.best_param
        # the best rewards stay 0-d tensors on the solver's device (tell() does not synchronise: the generation loop of
        # rollout.es_generation queues ask -> fit -> rollout -> tell without a host read); result() turns them into floats
        self._best_reward = torch.zeros((), dtype=dtype, device=self.device)
        self._curr_best_reward = torch.zeros((), dtype=dtype, device=self.device)
        self.first_iteration = True
        self.forget_best = forget_best
        self.weight_decay = weight_decay
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)

    def reset(self, param):
        self.best_param = torch.as_tensor(param, dtype=self.dtype, device=self.device).clone()
        self.curr_best_param = self.best_param.clone()
        self.first_iteration = True

    def rms_stdev(self):
        return self.sigma

    def ask(self, draws=None):
        """Returns solutions [popsize, num_params].  draws = (normal[pop,n], parents[pop,2] ints,
        mate_uniform[pop,n]) overrides the generator (parents/mate are unused on the first iteration)."""
        P, n = self.popsize, self.num_params
        if draws is None:
            normal = torch.randn(P, n, generator=self.gen, device=self.device, dtype=self.dtype)
            parents = torch.randint(0, max(self.elite_popsize, 1), (P, 2), generator=self.gen, device=self.device)
            mate_u = torch.rand(P, n, generator=self.gen, device=self.device, dtype=self.dtype)
        else:
            normal, parents, mate_u = [torch.as_tensor(d, device=self.device) for d in draws]
            normal, mate_u = normal.to(self.dtype), mate_u.to(self.dtype)
        self.epsilon = normal * self.sigma
        if self.first_iteration:
            solutions = self.best_param[None, :] + self.epsilon
        else:
            a = self.elite_params[parents[:, 0].long()]
            b = self.elite_params[parents[:, 1].long()]
            child = torch.where(mate_u > 0.5, b, a)          # mate(): c[idx] = b[idx] where rand > 0.5
            solutions = child + self.epsilon
        self.solutions = solutions
        return solutions

    def tell(self, reward_table_result):
        reward_table = torch.as_tensor(reward_table_result, dtype=self.dtype, device=self.device).clone()
        assert reward_table.numel() == self.popsize, "Inconsistent reward_table size reported."
        if self.weight_decay > 0:
            reward_table = reward_table - self.weight_decay * (self.solutions * self.solutions).mean(dim=1)
        if self.forget_best or self.first_iteration:
            reward, solution = reward_table, self.solutions
        else:
            reward = torch.cat([reward_table, self.elite_rewards])
            solution = torch.cat([self.solutions, self.elite_params])
        # alg/es.py:300 `np.argsort(reward)[::-1][0:elite_popsize]`: the REVERSE of an ascending sort, so among equal rewards the
        # later index comes first (a descending stable sort would put the earlier one first)
        idx = torch.argsort(reward, stable=True).flip(0)[: self.elite_popsize]
        self.elite_rewards = reward[idx]
        self.elite_params = solution[idx]
        self._curr_best_reward = self.elite_rewards[0].clone()
        self.curr_best_param = self.elite_params[0].clone()
        if self.first_iteration:
            self.first_iteration = False
            self._best_reward = self._curr_best_reward
            self.best_param = self.curr_best_param
        else:                                               # alg/es.py:308-311 `if curr_best_reward > best_reward`, as a select on the device
            better = self._curr_best_reward > self._best_reward
            self._best_reward = torch.where(better, self._curr_best_reward, self._best_reward)
            self.best_param = torch.where(better, self.curr_best_param, self.best_param)
        if self.sigma > self.sigma_limit:
            self.sigma *= self.sigma_decay

    @property
    def best_reward(self):
        return float(self._best_reward)

    @property
    def curr_best_reward(self):
        return float(self._curr_best_reward)

    def current_param(self):
        return self.elite_params[0]

    def set_mu(self, mu):
        pass

    def get_best_param(self):
        return self.best_param

    def result(self):
        return (self.best_param, self.best_reward, self.curr_best_reward, self.sigma, self.curr_best_param)


# ---------------------------------------------------------------------------------------------------------------------------
# PEPG / OpenES / SimpleES.  State (mu, PEPG's sigma vector, Adam's m / v, the best parameters and rewards) are tensors on the
# solver's device; the scalar sigma of OpenES / SimpleES, learning_rate and Adam's t are Python numbers that evolve without
# reading the device.  ask() and tell() read nothing back: every data-dependent branch of the reference is a torch.where.
#
# The arithmetic is the reference's, odd corners included: centered ranks are float32 and stay float32 through the in-place
# weight decay, so the mean / std / baseline taken of them are float32 reductions -- in numpy's order (_np_sum), because one
# float32 ulp in a mean moves mu by 1e-9, five orders above what the golden traces allow.
_PLANS = {}


def _pairwise_plan(n, device):
    """numpy's pairwise summation of n contiguous numbers as index tensors, built once per n and device: blocks of at most 128
    (a longer run is halved, the left half rounded down to a multiple of 8) are summed with 8 running accumulators and a
    sequential tail, and the block sums are added up the binary tree of the halvings.  Index n points at an appended zero."""
    key = (n, str(device))
    if key in _PLANS:
        return _PLANS[key]
    leaves, inner = [], []                                   # inner: [height, left id, right id]; leaf ids are >= 0, inner ones < 0

    def split(lo, m):                                       # -> (height, id)
        if m <= 128:
            leaves.append((lo, m))
            return 0, len(leaves) - 1
        h = m // 2 - (m // 2) % 8
        (ha, a), (hb, b) = split(lo, h), split(lo + h, m - h)
        inner.append([max(ha, hb) + 1, a, b])
        return inner[-1][0], -len(inner)
    split(0, n)
    rows, tails = max(m // 8 for _, m in leaves), max(m % 8 for _, m in leaves)
    main = [[[lo + 8 * r + j if r < m // 8 else n for j in range(8)] for r in range(rows)] for lo, m in leaves]
    tail = [[lo + m - m % 8 + j if j < m % 8 else n for j in range(tails)] for lo, m in leaves]
    # the inner nodes by height, so that a level's children are already in the value buffer [leaves | level 1 | level 2 | ...]
    order = sorted(range(len(inner)), key=lambda i: inner[i][0])
    slot = {-(i + 1): len(leaves) + k for k, i in enumerate(order)}
    levels = []
    for height in sorted({nd[0] for nd in inner}):
        level = [inner[i] for i in order if inner[i][0] == height]
        levels.append(tuple(torch.tensor([c if c >= 0 else slot[c] for c in (nd[k] for nd in level)], device=device) for k in (1, 2)))
    as_index = lambda a, w: torch.tensor(a, dtype=torch.long, device=device).reshape(len(leaves), -1, w) if w else None
    _PLANS[key] = (as_index(main, 8) if rows else None, as_index(tail, tails), levels)
    return _PLANS[key]


def _np_sum(x):
    """Sum of a 1-D tensor in the order numpy's add.reduce takes (see _pairwise_plan): bit-equal to np.sum of the same numbers."""
    n = x.numel()
    if n > 8192:                                            # numpy hands add.reduce at most its buffer size (8192 elements) at a time
        total = x.new_zeros(())
        for lo in range(0, n, 8192):
            total = total + _np_sum(x.reshape(-1)[lo:lo + 8192])
        return total
    main, tail, levels = _pairwise_plan(n, x.device)
    xp = torch.cat([x.reshape(-1), x.new_zeros(1)])
    if main is not None:
        blk = xp[main]                                      # [leaves, rows, 8]
        r = blk[:, 0]
        for k in range(1, blk.shape[1]):
            r = r + blk[:, k]
        vals = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
    else:
        vals = x.new_zeros(1)
    if tail is not None:
        t = xp[tail[:, 0]]                                  # [leaves, tails]
        for j in range(t.shape[1]):
            vals = vals + t[:, j]
    for left, right in levels:
        vals = torch.cat([vals, vals[left] + vals[right]])
    return vals[-1]


def _div(x, d):
    """x / d rounded once in x's precision, whatever the device makes of a float32 division or of a division by a host number:
    the quotient is taken in float64, and rounding that to float32 gives the correctly rounded float32 quotient"""
    return (x.double() / (d.double() if torch.is_tensor(d) else d)).to(x.dtype)


def _np_mean(x):
    return _div(_np_sum(x), x.numel())


def _np_std(x):
    d = x - _np_mean(x)
    var = _div(_np_sum(d * d), x.numel())
    return torch.sqrt(var.double()).to(var.dtype)           # as _div: the float32 root by way of float64


def compute_centered_ranks(x):
    """alg/es.py:9-27: ranks in [0, n) scaled to [-0.5, 0.5], float32.  Equal values rank in index order (a stable ascending
    sort; the reference's x.argsort() leaves their order undefined)."""
    x = x.reshape(-1)
    n = x.numel()
    order = torch.argsort(x, stable=True)
    ranks = torch.empty_like(order).scatter_(0, order, torch.arange(n, device=x.device))
    return _div(ranks.to(torch.float32), n - 1) - 0.5


class Adam:
    """alg/es.py:36-49, 76-90: the optimizer OpenES and PEPG move `pi.mu` with.  m and v are tensors, t a Python number."""

    def __init__(self, pi, stepsize, beta1=0.99, beta2=0.999, epsilon=1e-08):
        self.pi, self.stepsize, self.beta1, self.beta2, self.epsilon = pi, stepsize, beta1, beta2, epsilon
        self.t = 0
        self.m = torch.zeros(pi.num_params, dtype=pi.dtype, device=pi.device)
        self.v = torch.zeros(pi.num_params, dtype=pi.dtype, device=pi.device)

    def update(self, globalg):
        self.t += 1
        a = self.stepsize * math.sqrt(1 - self.beta2 ** self.t) / (1 - self.beta1 ** self.t)
        self.m = self.beta1 * self.m + (1 - self.beta1) * globalg
        self.v = self.beta2 * self.v + (1 - self.beta2) * (globalg * globalg)
        self.pi.mu = self.pi.mu + -a * self.m / (torch.sqrt(self.v) + self.epsilon)


class _MuSolver:
    """What the three solvers around a mean `mu` share: device state, draws, weight decay, the best-so-far bookkeeping."""

    def _setup(self, num_params, popsize, weight_decay, forget_best, param, device, seed, dtype):
        self.num_params, self.popsize = int(num_params), int(popsize)
        self.device, self.dtype = torch.device(device), dtype
        self.weight_decay, self.forget_best = weight_decay, forget_best
        self.mu = torch.zeros(self.num_params, dtype=dtype, device=self.device) if param is None else \
            torch.as_tensor(param, dtype=dtype, device=self.device).clone()
        self.best_mu = self.mu.clone()
        self.curr_best_mu = self.mu.clone()
        self._best_reward = torch.zeros((), dtype=dtype, device=self.device)
        self._curr_best_reward = torch.zeros((), dtype=dtype, device=self.device)
        self.first_iteration = True
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)
        for n in (self.popsize, self.popsize - 1):            # tell()'s summation plans, so that tell() copies nothing to the device
            for m in {min(n, 8192), n % 8192 if n > 8192 else 0} - {0}:
                _pairwise_plan(m, self.device)

    def _normal(self, rows, draws):
        if draws is None:
            return torch.randn(rows, self.num_params, generator=self.gen, device=self.device, dtype=self.dtype)
        normal = torch.as_tensor(draws, device=self.device).to(self.dtype)
        assert normal.shape == (rows, self.num_params), "draws must be [%d, %d]" % (rows, self.num_params)
        return normal

    def _rewards(self, fitness, rank_fitness):
        """np.array(fitness), the rank transform and `reward += l2_decay` (alg/es.py:29-31): in place there, so ranks stay float32"""
        reward = torch.as_tensor(fitness, device=self.device).to(self.dtype).reshape(-1)
        assert reward.numel() == self.popsize, "Inconsistent reward_table size reported."
        if rank_fitness:
            reward = compute_centered_ranks(reward)
        if self.weight_decay > 0:
            l2_decay = -self.weight_decay * (self.solutions * self.solutions).mean(dim=1)
            reward = (reward + l2_decay).to(reward.dtype)
        return reward

    def _keep_best(self, reward, mu):
        self._curr_best_reward, self.curr_best_mu = reward, mu
        if self.first_iteration or self.forget_best:
            self.first_iteration = False
            self._best_reward, self.best_mu = reward, mu
        else:                                               # `curr_best_reward > best_reward` as a select on the device
            better = reward > self._best_reward
            self._best_reward = torch.where(better, reward, self._best_reward)
            self.best_mu = torch.where(better, mu, self.best_mu)

    @property
    def best_reward(self):
        return float(self._best_reward)

    @property
    def curr_best_reward(self):
        return float(self._curr_best_reward)

    def current_param(self):
        return self.curr_best_mu

    def set_mu(self, mu):
        self.mu = torch.as_tensor(mu, dtype=self.dtype, device=self.device).clone()

    def best_param(self):
        return self.best_mu

    get_best_param = best_param                             # the name SimpleGA and the examples use

    def result(self):
        return (self.best_mu, self.best_reward, self.curr_best_reward, self.sigma)


class SimpleES(_MuSolver):
    """alg/es.py:145-211: mu becomes the softmax-weighted mean of the population (rewards scaled to [0, 3])."""

    def __init__(self, num_params, popsize=256, sigma_init=0.1, sigma_decay=0.999, sigma_limit=0.01, weight_decay=0.01,
                 param=None, device="cpu", seed=0, dtype=torch.float64):
        self._setup(num_params, popsize, weight_decay, False, param, device, seed, dtype)
        self.sigma, self.sigma_init, self.sigma_decay, self.sigma_limit = sigma_init, sigma_init, sigma_decay, sigma_limit

    def rms_stdev(self):
        return self.sigma

    def ask(self, draws=None):
        """Returns solutions [popsize, num_params]; draws = the standard-normal [popsize, num_params] to use instead of the generator."""
        self.epsilon = self._normal(self.popsize, draws)
        self.solutions = self.mu[None, :] + self.epsilon * self.sigma
        return self.solutions

    def tell(self, fitness):
        reward = self._rewards(fitness, False)
        top = torch.argsort(reward, stable=True)[-1:]        # the last of equals, as in SimpleGA.tell
        self._keep_best(reward[top][0], self.solutions[top][0])
        if self.sigma > self.sigma_limit:
            self.sigma *= self.sigma_decay
        min_r = reward.min()
        dis = reward.max() - min_r
        reward = torch.where(dis > 1e-2, 3 * (reward - min_r) / dis, reward)
        exp_reward = torch.exp(reward)
        self.mu = (exp_reward / _np_sum(exp_reward)) @ self.solutions


class OpenES(_MuSolver):
    """alg/es.py:328-444.  tell() moves mu twice, as the reference does: by learning_rate * change_mu, then by the Adam step."""

    def __init__(self, num_params, sigma_init=0.1, sigma_decay=0.999, sigma_limit=0.01, learning_rate=0.01,
                 learning_rate_decay=0.9999, learning_rate_limit=0.001, popsize=256, antithetic=False, weight_decay=0.01,
                 rank_fitness=True, forget_best=True, param=None, device="cpu", seed=0, dtype=torch.float64):
        self.antithetic = antithetic
        if antithetic:
            assert popsize % 2 == 0, "Population size must be even"
            self.half_popsize = int(popsize / 2)
        self.rank_fitness = rank_fitness
        self._setup(num_params, popsize, weight_decay, forget_best or rank_fitness, param, device, seed, dtype)   # ranking forgets the best
        self.sigma, self.sigma_init, self.sigma_decay, self.sigma_limit = sigma_init, sigma_init, sigma_decay, sigma_limit
        self.learning_rate, self.learning_rate_decay, self.learning_rate_limit = learning_rate, learning_rate_decay, learning_rate_limit
        self.optimizer = Adam(self, learning_rate)

    def rms_stdev(self):
        return self.sigma

    def ask(self, draws=None):
        """Returns solutions [popsize, num_params]; draws = the standard-normal array to use instead of the generator:
        [popsize / 2, num_params] when antithetic (the second half of the population mirrors the first), else [popsize, num_params]."""
        if self.antithetic:
            half = self._normal(self.half_popsize, draws)
            self.epsilon = torch.cat([half, -half])
        else:
            self.epsilon = self._normal(self.popsize, draws)
        self.solutions = self.mu[None, :] + self.epsilon * self.sigma
        return self.solutions

    def tell(self, fitness):
        reward = self._rewards(fitness, self.rank_fitness)
        top = torch.argsort(reward, stable=True)[-1:]
        self._keep_best(reward[top][0], self.solutions[top][0])
        normalized_reward = _div(reward - _np_mean(reward), _np_std(reward))
        change_mu = 1. / (self.popsize * self.sigma) * (normalized_reward.to(self.dtype) @ self.epsilon)
        self.mu = self.mu + self.learning_rate * change_mu
        self.optimizer.stepsize = self.learning_rate
        self.optimizer.update(-change_mu)
        if self.sigma > self.sigma_limit:
            self.sigma *= self.sigma_decay
        if self.learning_rate > self.learning_rate_limit:
            self.learning_rate *= self.learning_rate_decay


class PEPG(_MuSolver):
    """alg/es.py:446-619, with a standard deviation per parameter.  As there: the first tell() resets sigma to sigma_init;
    elite_ratio > 0 moves mu to the mean of the elite's offsets instead of the gradient step (the `ses` setting); the gradient
    step moves mu twice, by the Adam step and by learning_rate * change_mu; average_baseline=False wants an odd population whose
    candidate 0 is mu itself.  One thing is not carried over: where the reference's best_mu is `self.mu` itself (that baseline
    candidate winning) and mu is then moved in place, its best_mu moves along; here best_mu is the mu that was evaluated."""

    def __init__(self, num_params, sigma_init=0.10, sigma_alpha=0.20, sigma_decay=0.999, sigma_limit=0.01, sigma_max_change=0.2,
                 learning_rate=0.01, learning_rate_decay=0.9999, learning_rate_limit=0.01, elite_ratio=0, popsize=256,
                 average_baseline=True, weight_decay=0.01, rank_fitness=True, forget_best=True, param=None, device="cpu",
                 seed=0, dtype=torch.float64):
        self.average_baseline = average_baseline
        if average_baseline:
            assert popsize % 2 == 0, "Population size must be even"
            self.batch_size = int(popsize / 2)
        else:
            assert popsize & 1, "Population size must be odd"
            self.batch_size = int((popsize - 1) / 2)
        self.rank_fitness = rank_fitness
        self._setup(num_params, popsize, weight_decay, forget_best or rank_fitness, param, device, seed, dtype)
        self.sigma_init, self.sigma_alpha, self.sigma_decay = sigma_init, sigma_alpha, sigma_decay
        self.sigma_limit, self.sigma_max_change = sigma_limit, sigma_max_change
        self.learning_rate, self.learning_rate_decay, self.learning_rate_limit = learning_rate, learning_rate_decay, learning_rate_limit
        self.elite_ratio = elite_ratio
        self.elite_popsize = int(self.popsize * self.elite_ratio)
        self.use_elite = self.elite_popsize > 0
        self.sigma = torch.full((self.num_params,), sigma_init, dtype=dtype, device=self.device)
        self.optimizer = Adam(self, learning_rate)

    def rms_stdev(self):
        """mean(sqrt(sigma * sigma)) as a 0-d tensor on the solver's device"""
        return torch.sqrt(self.sigma * self.sigma).mean()

    def ask(self, draws=None):
        """Returns solutions [popsize, num_params]: mu + epsilon, mu - epsilon (after mu itself when average_baseline is off);
        draws = the standard-normal [batch_size, num_params] to use instead of the generator."""
        self.epsilon = self._normal(self.batch_size, draws) * self.sigma[None, :]
        self.epsilon_full = torch.cat([self.epsilon, -self.epsilon])
        epsilon = self.epsilon_full if self.average_baseline else torch.cat([torch.zeros_like(self.epsilon[:1]), self.epsilon_full])
        self.solutions = self.mu[None, :] + epsilon
        return self.solutions

    def tell(self, fitness):
        reward_table = self._rewards(fitness, self.rank_fitness)
        if self.average_baseline:
            b, reward = _np_mean(reward_table), reward_table
        else:
            b, reward = reward_table[0], reward_table[1:]
        idx = torch.argsort(reward, stable=True).flip(0)
        if self.use_elite:
            idx = idx[:self.elite_popsize]
        best_reward = reward[idx[:1]][0]
        best_mu = self.mu + self.epsilon_full[idx[:1]][0]
        if not self.average_baseline:                       # `best_reward > b`: else mu itself was the best candidate
            better = best_reward > b
            best_mu = torch.where(better, best_mu, self.mu)
            best_reward = torch.where(better, best_reward, b)
        if self.first_iteration:
            self.sigma = torch.full_like(self.sigma, self.sigma_init)
        self._keep_best(best_reward, best_mu)
        epsilon, sigma, B = self.epsilon, self.sigma, self.batch_size
        if self.use_elite:
            self.mu = self.mu + self.epsilon_full[idx].mean(dim=0)
        else:
            rT = reward[:B] - reward[B:]
            change_mu = rT.to(self.dtype) @ epsilon
            self.optimizer.stepsize = self.learning_rate
            self.optimizer.update(-change_mu)
            self.mu = self.mu + change_mu * self.learning_rate
        if self.sigma_alpha > 0:
            stdev_reward = 1.0 if self.rank_fitness else _np_std(reward)
            S = (epsilon * epsilon - (sigma * sigma)[None, :]) / sigma[None, :]
            reward_avg = (reward[:B] + reward[B:]) / 2.0
            rS = reward_avg - b
            delta_sigma = (rS.to(self.dtype) @ S) / (2 * B * stdev_reward)
            change_sigma = self.sigma_alpha * delta_sigma
            change_sigma = torch.minimum(change_sigma, self.sigma_max_change * sigma)
            change_sigma = torch.maximum(change_sigma, -self.sigma_max_change * sigma)
            self.sigma = sigma + change_sigma
        if self.sigma_decay < 1:
            self.sigma = torch.where(self.sigma > self.sigma_limit, self.sigma * self.sigma_decay, self.sigma)
        if self.learning_rate_decay < 1 and self.learning_rate > self.learning_rate_limit:
            self.learning_rate *= self.learning_rate_decay


ALGS = ("ga", "ses", "pepg", "openes", "simples")


def make_solver(alg, num_params, popsize, sigma, sigma_decay, param=None, device="cpu", seed=0):
    """The solver of `Dynamic_train.py --alg`, with the settings of ES_ParallelModel.set_solver
    (model/Dynamic_parallel_model.py:102-149): ga = SimpleGA, ses = PEPG taking the elite-mean step, pepg, openes (antithetic),
    simples = SimpleES."""
    common = dict(sigma_init=sigma, sigma_decay=sigma_decay, sigma_limit=0.02, weight_decay=0.005, popsize=popsize, param=param,
                  device=device, seed=seed)
    if alg == "ga":
        return SimpleGA(num_params, elite_ratio=0.1, **common)
    if alg == "ses":
        return PEPG(num_params, sigma_alpha=0.2, elite_ratio=0.1, **common)
    if alg == "pepg":
        return PEPG(num_params, sigma_alpha=0.20, learning_rate=0.01, learning_rate_decay=1.0, learning_rate_limit=0.01, **common)
    if alg == "openes":
        return OpenES(num_params, learning_rate=0.01, learning_rate_decay=1.0, learning_rate_limit=0.01, antithetic=True, **common)
    if alg == "simples":
        return SimpleES(num_params, **common)
    if alg == "cma":
        raise ValueError("--alg cma wraps the `cma` package (alg/es.py:92-143), which this project does not depend on; "
                         "choose one of " + ", ".join(ALGS))
    raise ValueError("unknown solver %r: choose one of %s" % (alg, ", ".join(ALGS)))
