"""A run with no device behind it, for the step loops of lammps_mtp_kokkos_amd.md (tests/test_relax_cpu.py: _minimise_pass;
tests/test_sample_cpu.py: _sample_pass)."""


class StubRun:
    """a run that only writes down what a step loop asks of it: F forces, C capture, M the monitor read, B rebuild, and the
    driver's own launches, S the minimiser step, I and H the sampler's first and second half; `answers` are the (nothing runs any
    more, lists are stale) replies of the reads, in order, (False, False) once they run out"""

    def __init__(self, answers=()):
        self.log, self.answers, self.moves, self.graded_forces, self.recorded = [], list(answers), 0, [], []

    def forces(self, grade):
        self.log.append("F")
        self.graded_forces.append(bool(grade))

    def capture(self, step):
        self.log.append("C%d" % step)

    def step(self, s, last):
        self.log.append("S%d%s" % (s, "last" if last else ""))

    def first_half(self, s):
        self.log.append("I%d" % s)

    def second_half(self, s, kick):
        self.log.append("H%d" % s)
        assert bool(kick) == (s > 0)                                                 # step 0 is the thermostat's setup: no kick

    def record(self, s):
        self.recorded.append(s)

    def moved(self):
        self.moves += 1

    def read(self):
        self.log.append("M")
        return self.answers.pop(0) if self.answers else (False, False)

    def reneighbor(self):
        self.log.append("B")
