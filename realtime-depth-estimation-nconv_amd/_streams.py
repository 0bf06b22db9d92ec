"""Side streams: the one cache and the two fork / join forms of every multi-stream path. What
hipGraph capture needs of them ("Streams under hipGraph capture") is enforced here:
(1) a stream is made once per (purpose, device, count) and never dropped, so it outlives every
graph that captured work on it, and no Event is held across calls (forks and joins are
wait_stream); (2) every fork is joined before the forking stream goes on; (3) a tensor made on a
side stream and read on the forking one is handed over with record_stream -- anything else that
crosses streams is allocated before the fork."""
import torch

_STREAMS = {}


def side_streams(purpose, device, n):
    """The n side streams of one purpose on one device (a purpose per multi-stream path: no two
    paths share a stream)."""
    key = (purpose, device.index, n)
    if key not in _STREAMS:
        _STREAMS[key] = [torch.cuda.Stream(device=device) for _ in range(n)]
    return _STREAMS[key]


def fork_join(purpose, device, bounds, fn):
    """fn(b0, b1) for every batch slice bounds[k]:bounds[k + 1] -- slice 0 on the current stream,
    slice k on the purpose's side stream k - 1, empty slices skipped -- after the work the current
    stream holds so far, joined before returning. Returns the slices' results (None for a skipped
    slice); a side-stream slice returns None or the tensors it allocated (a sequence), which are
    handed over to the current stream here."""
    cur = torch.cuda.current_stream(device)
    side = side_streams(purpose, device, len(bounds) - 2)
    for st in side:
        st.wait_stream(cur)
    res = []
    for k, st in enumerate([cur] + side):
        b0, b1 = bounds[k], bounds[k + 1]
        if b1 == b0:
            res.append(None)
            continue
        with torch.cuda.stream(st):
            res.append(fn(b0, b1))
    for st in side:
        cur.wait_stream(st)
    for r in res[1:]:
        for t in r or ():
            t.record_stream(cur)
    return res


class SideStream:
    """Work beside the current stream on the purpose's one side stream: fork() orders the side
    stream after what the current stream holds so far and returns it (enqueue on it under
    torch.cuda.stream); join(*tensors made there) orders the current stream after it."""

    def __init__(self, purpose, device):
        self.cur, self.stream = torch.cuda.current_stream(device), side_streams(purpose, device, 1)[0]

    def fork(self):
        self.stream.wait_stream(self.cur)
        return self.stream

    def join(self, *made):
        self.cur.wait_stream(self.stream)
        for t in made:
            t.record_stream(self.cur)
