"""Python restatement of a stream's frame sync (lsn_stream_frame_sync), written from the definition in include/ltesniffer_amd.h / DESIGN.md section 3.1m: the
decision over one PBCH attempt and the rule that says which segments are attempted, when a result is looked at, and what the TTI and the hold are from then on.
Shares no code with the library."""

DELAY = 2               # the attempt of segment a is looked at on entering segment a + 2
TRIES = 8               # the default: four radio frames, one PBCH period
WRAP = 10240


def decide(mib, nof_prb, nof_ports, counted):
    """mib: None (not found, or not launched) or a dict with found, sfn, nof_prb, nof_ports; counted: the TTI the attempt's subframe was counted as
    -> (accepted, delta signed in (-5120, 5120])"""
    if not mib or not mib["found"] or mib["nof_prb"] != nof_prb or mib["nof_ports"] != nof_ports:
        return False, 0
    assert counted % 5 == 0, "a segment that does not begin on a TTI multiple of 5"
    delta = (10 * mib["sfn"] - counted) % WRAP
    if delta > WRAP // 2:
        delta -= WRAP
    assert delta % 5 == 0
    return True, delta


class Rule:
    """one cell.  For every segment h, in order: entered(h, jumped, result) - jumped: a jump of re-acquisition is in force at this segment; result(a) -> the MIB
    dict of segment a's attempt, asked only for an attempt that was launched and that somebody waits for - and then launched(h, gap) once the segment's first piece
    goes out (gap: the first subframe's input span reads a declared gap).  After entered(h): tti(sf) of the segment's subframes, holding"""

    def __init__(self, nof_prb, nof_ports, start_tti=0, tries=0, hold=True):
        self.nof_prb, self.nof_ports, self.start_tti, self.tries, self.hold = nof_prb, nof_ports, start_tti, tries or TRIES, hold
        self.first_nsf = 5 - start_tti % 5
        self.active, self.g, self.shift, self.h = False, 0, 0, None
        self.due = {}           # segment -> launched, for the segments that were due an attempt
        self.status = dict(checks=0, attempts=0, confirmed=0, relabelled=0, given_up=0, accept_segment=0, relabel_segment=0, last_sfn=0, last_delta=0, shift=0)

    def segment_start(self, a):
        return self.first_nsf + 5 * (a - 1) if a else 0

    def entered(self, h, jumped, result):
        st = self.status
        a = h - DELAY
        if a in self.due:
            was_launched = self.due.pop(a)
            if self.active and a >= self.g:                # in front of the running check's first segment: ignored
                counted = (self.start_tti + self.segment_start(a) + self.shift) % WRAP
                mib = result(a) if was_launched else None
                ok, delta = decide(mib, self.nof_prb, self.nof_ports, counted)
                if ok:
                    st["last_sfn"], st["last_delta"], st["accept_segment"] = mib["sfn"], delta, a
                    if delta:
                        self.shift = (self.shift + delta) % WRAP
                        st["relabelled"] += 1
                        st["relabel_segment"] = h
                    else:
                        st["confirmed"] += 1
                    self.active = False
                elif a - self.g + 1 >= self.tries:
                    st["given_up"] += 1
                    self.active = False
        if jumped:                                         # behind the result of two segments ago: a new jump restarts the check at its own g
            self.active, self.g = True, h
            st["checks"] += 1
        self.h = h
        st["shift"] = self.shift

    @property
    def holding(self):
        return self.active and self.hold

    def tti(self, sf):
        return (self.start_tti + sf + self.shift) % WRAP

    def launched(self, h, gap=False):
        """-> the segment is due an attempt"""
        assert h == self.h
        if not (self.active and self.g <= h < self.g + self.tries):
            return False
        self.due[h] = not gap
        self.status["attempts"] += 0 if gap else 1
        return True
