"""Model of the chunked flatten stage (tudocomp_amd/csrc/flatten.hip, flatten_factors with chunks > 1).

`position_space.flatten_rounds` visits every waiting factor in every round.  A chain step that lands in factor s needs the FINAL
source of s only if s has a lower rank than the walking factor (`s < i`), and the original one otherwise: the final source of rank i
depends on final sources of ranks < i alone.  So the same round loop may run on the rank range [r_0, r_1) until it is done, then on
[r_1, r_2), ... with r_k = z k / K, and every range is final when its own rounds are over -- whatever lies behind it.  That is what
lets the pack and the download of a range's tiles start while the next range is still being flattened."""


def chunk_bounds(z, K):
    """the rank bounds r_0 .. r_K of K ranges of equal counts (K clamped to 1 .. z, as the device does)"""
    K = max(1, min(K, z))
    return [z * k // K for k in range(K + 1)]


def flatten_rounds_chunked(factors, K):
    """factors: list of (pos, src, len) sorted by pos; K: rank ranges, done one after the other.
    Returns (new factor list, num_flattened, max_depth_lb, rounds summed over the ranges)."""
    z = len(factors)
    if z == 0:
        return [], 0, 0, 0
    end = factors[-1][0] + factors[-1][2]
    owner = [-1] * end
    for i, (pos, src, ln) in enumerate(factors):
        for j in range(ln):
            owner[pos + j] = i
    orig_src = [f[1] for f in factors]
    final_src = list(orig_src)
    done = [False] * z
    cur_src = list(orig_src)
    depth = [0] * z
    rounds = 0
    bounds = chunk_bounds(z, K)
    for r0, r1 in zip(bounds, bounds[1:]):
        assert all(done[:r0]) and r1 > r0
        while not all(done[r0:r1]):
            rounds += 1
            snapshot = list(done)
            for i in range(r0, r1):
                if done[i]:
                    continue
                pos, _, ln = factors[i]
                src = cur_src[i]
                while True:
                    if src >= end or owner[src] < 0:
                        done[i] = True
                        break
                    s = owner[src]
                    spos, _, slen = factors[s]
                    d = src - spos
                    if d + ln > slen:
                        done[i] = True
                        break
                    if s < i:
                        if not snapshot[s]:
                            break           # wait for s: it lies in this range (every earlier range is done)
                        assert s >= r0 or done[s]
                        ssrc = final_src[s]
                    else:
                        ssrc = orig_src[s]  # s >= i, in this range or a later one: the original value
                    src = ssrc + d
                    depth[i] += 1
                cur_src[i] = src
                if done[i]:
                    final_src[i] = src if depth[i] else orig_src[i]
    out = [(f[0], final_src[i], f[2]) for i, f in enumerate(factors)]
    nf = sum(1 for d in depth if d)
    return out, nf, max(depth), rounds
