"""CPU reference of prompt-lookup decoding in plain Python: the draft rule, the accept rule, one whole call of
ops.lookup_accept on CPU tensors, and the trace of a generation as a function of its final ids.  No mmgl_amd import."""
import torch


def draft(hist, K, N):
    """The drafts behind the history `hist` (a list): for n = min(N, len - 1) down to 1, the latest p <= len - n - 1 with
    hist[p:p+n] == hist[-n:] gives hist[p+n : p+n+K] (at least one token, cut at the history's end); no match: []."""
    L = len(hist)
    for n in range(min(N, L - 1), 0, -1):
        pat = hist[L - n:]
        for p in range(L - n - 1, -1, -1):
            if hist[p:p + n] == pat:
                return hist[p + n:p + n + K]
    return []


def accept(argmax, drafts, gen, n_new, eos=None):
    """argmax[i]: the greedy token behind block input i (input 0 is the row's last token, input i >= 1 is drafts[i - 1]).  Returns
    (emitted tokens, finished): e_0 = a_0, e_i = a_i while i <= len(drafts) and drafts[i - 1] == e_{i-1}; stops behind eos and at
    n_new tokens, either of which finishes the row."""
    out = []
    for i, a in enumerate(argmax):
        if i > 0 and not (i <= len(drafts) and drafts[i - 1] == out[-1]):
            break
        out.append(int(a))
        if eos is not None and out[-1] == eos:
            return out, True
        if gen + len(out) >= n_new:
            return out, True
    return out, False


def lookup_accept_ref(logits, m_in, block, n_draft, ids, prompt_mask, gen, lens, finished, n_new, N, eos=None, pad=None, pos_offset=0,
                      pos_max=2 ** 31 - 1):
    """One call of ops.lookup_accept on CPU tensors; nothing is changed in place.  Returns a dict of the tensors after the call:
    block, n_draft, positions, ids, gen, lens, finished, emitted."""
    B, M1 = block.shape
    K = M1 - 1
    T = ids.shape[1] - n_new
    V = logits.shape[1]
    am = logits.float().view(B, m_in, V)
    out = dict(block=block.clone(), n_draft=n_draft.clone(), positions=torch.zeros(B, M1, dtype=torch.int64), ids=ids.clone(),
               gen=gen.clone(), lens=lens.clone(), finished=finished.clone(), emitted=torch.zeros(B, dtype=torch.int32))
    for b in range(B):
        g = int(gen[b])
        fin = bool(finished[b]) or g >= n_new
        toks = []
        if not fin:
            nd = min(max(int(n_draft[b]), 0), m_in - 1) if m_in > 1 else 0
            arg = [_argmax(am[b, i]) for i in range(m_in)]
            toks, fin = accept(arg, block[b, 1:1 + nd].tolist(), g, n_new, eos)
        k = len(toks)
        for i, t in enumerate(toks):
            out["ids"][b, T + g + i] = t
        g_after = g + k
        if k and eos is not None and toks[-1] == eos:
            out["ids"][b, T + g + k:] = pad
            g_after = n_new
        out["emitted"][b] = k
        out["gen"][b] = g_after
        if m_in > 1:
            out["lens"][b] += k
        out["finished"][b] = int(fin)
        hist = [int(t) for t, a in zip(ids[b, :T].tolist(), prompt_mask[b].tolist()) if a] + out["ids"][b, T:T + g + k].tolist()
        n_valid = len(hist) - (g + k)
        t_last = toks[-1] if k else int(block[b, 0])
        d = [] if fin else draft(hist, K, N)
        out["block"][b] = torch.tensor([t_last] + d + [t_last] * (K - len(d)))
        out["n_draft"][b] = len(d)
        p0 = n_valid + pos_offset + g_after - 1
        out["positions"][b] = torch.tensor([min(max(p0 + i, 0), pos_max) for i in range(M1)])
    return out


def _argmax(row):
    """Lowest index of the largest non-NaN value; 0 for a row of NaN only."""
    row = torch.where(torch.isnan(row), torch.full_like(row, float("-inf")), row)
    return int(torch.argmax(row))          # torch.argmax returns the first maximal index


def simulate(valid_prompt, new_tokens, K, N, eos=None):
    """The trace of the generation that returned `new_tokens` (the row's n_new new tokens: greedy tokens, then pads behind an EOS)
    for the prompt whose valid tokens are `valid_prompt`: greedy decoding's token behind any accepted prefix is the next token of the
    result, so the trace is a pure function of the final ids.  Returns a list with one dict per call the row takes part in (call 0 is
    the prefill's): k = tokens emitted, nd = drafts it verified, eos_at = index inside the call's tokens where EOS fell (or None)."""
    n_new = len(new_tokens)
    real = list(new_tokens)
    if eos is not None and eos in real:
        real = real[:real.index(eos) + 1]
    hist, g, calls, drafts = list(valid_prompt), 0, [], []
    while g < len(real):
        toks, _ = accept(real[g:g + len(drafts) + 1], drafts, g, n_new, eos)
        calls.append(dict(k=len(toks), nd=len(drafts), eos_at=toks.index(eos) if eos is not None and eos in toks else None))
        hist += toks
        g += len(toks)
        drafts = draft(hist, K, N)
    return calls


def emitted_matrix(traces, steps):
    """int32 [steps + 1, B] from the per-row traces: a row that has finished emits 0."""
    out = torch.zeros(steps + 1, len(traces), dtype=torch.int32)
    for b, tr in enumerate(traces):
        for c, call in enumerate(tr):
            out[c, b] = call["k"]
    return out
