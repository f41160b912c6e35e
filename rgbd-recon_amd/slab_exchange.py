"""The slab exchange's bookkeeping for the torch.distributed path: the Python twin of csrc/slab_exchange.hpp (SlabRoles, GatherBook), event for
event and name for name -- the comments there say what each means.  Standard library only.  tests/test_slab_exchange.py replays the same event
scripts through both and compares every decision.  Python's integers do not wrap: the results equal the header's uint32_t arithmetic where m * 3
stays below 2^32, which m <= view pixels + 1 <= 16384^2 + 1 guarantees."""

NONE = -1


class SlabRoles:
    def __init__(self, rank=0, world=1, dedicated=False):
        self.rank, self.world, self.dedicated = rank, world, bool(dedicated)

    @property
    def worker(self): return not (self.dedicated and self.rank == 0)
    @property
    def first_worker(self): return 1 if self.dedicated else 0
    @property
    def gathers(self): return self.rank == 0

    def below(self): return (self.rank - 1, 1) if self.worker and self.rank > self.first_worker else (NONE, 0)      # (row, face) of the gathered halo
    def above(self): return (self.rank + 1, 0) if self.worker and self.rank < self.world - 1 else (NONE, 0)

    @property
    def own_in_parts(self): return self.rank == 0
    def exports(self, first): return self.worker and (first or self.rank != 0)
    def export_records(self, npx, cap): return npx if self.rank == 0 else cap
    @property
    def grouped(self): return self.world > 1
    def recv_begin(self): return 1 if self.rank == 0 else self.world
    def send_to(self): return NONE if self.rank == 0 else 0
    @staticmethod
    def exchange_floats(cap): return 8 + cap * 8
    @staticmethod
    def row_floats(npx): return 8 + npx * 8


class GatherBook:
    LAG = 2
    RING = LAG + 1
    VERDICTS = 64
    VERDICT, COMPARE, NOT_GATHERED, NOT_KEPT = range(4)           # status(): the four answers

    def __init__(self, min_capacity=4096, max_capacity=0):
        self.min_capacity, self.max_capacity = int(min_capacity), int(max_capacity)
        self.regathers = self.overflowed_frames = 0
        self._reset_frames()

    def _reset_frames(self):
        self.frame_no = 0
        self.last = None                                          # (frame, capacity) of the latest frame, until finish() has checked it
        self.caps = [0] * self.RING
        self.counts_rec = [False] * self.RING
        self.verdicts = [None] * self.VERDICTS                    # (frame, truncated)

    def recorded(self, slot): return self.counts_rec[slot]
    def open_slot(self): return self.frame_no % self.RING
    def lagged_slot(self): return NONE if self.frame_no < self.LAG else (self.frame_no - self.LAG) % self.RING
    def pending_slot(self): return NONE if self.last is None else self.last[0] % self.RING

    def _set_verdict(self, f, truncated):
        self.verdicts[f % self.VERDICTS] = (f, bool(truncated))

    def open(self, view_px, m):
        npx = min(self.max_capacity, view_px) if self.max_capacity else view_px
        if self.frame_no < self.LAG:
            return npx
        f = self.frame_no - self.LAG
        truncated = m > self.caps[f % self.RING]
        if truncated:
            self.overflowed_frames += 1
        self._set_verdict(f, truncated)
        cap = max(self.min_capacity, ((m * 3) // 2 + 1024 + 1023) // 1024 * 1024)
        return min(cap, npx)

    def queued(self, cap):
        slot = self.open_slot()
        self.counts_rec[slot], self.caps[slot] = True, cap
        self.last = (self.frame_no, cap)
        self.frame_no += 1

    def finish(self, view_px, m):
        """(regather, capacity)"""
        if self.last is None:
            return False, 0
        (f, cap), self.last, fix = self.last, None, (False, 0)
        if m > cap:
            self.regathers += 1
            fix = (True, min(view_px, m))
            self.caps[f % self.RING] = fix[1]
        self._set_verdict(f, False)
        return fix

    def status(self, f):
        """(kind, truncated, slot, capacity)"""
        if f >= self.frame_no:
            return self.NOT_GATHERED, 0, NONE, 0
        v = self.verdicts[f % self.VERDICTS]
        if v is not None and v[0] == f:
            return self.VERDICT, int(v[1]), NONE, 0
        if f + self.RING >= self.frame_no:
            return self.COMPARE, 0, f % self.RING, self.caps[f % self.RING]
        return self.NOT_KEPT, 0, NONE, 0

    def set_limits(self, min_records, max_records):
        self.min_capacity, self.max_capacity = int(min_records), int(max_records)

    def released(self):
        self._reset_frames()
