"""CPU oracle for the volpick sliding-window phase-picking path.

TEST INFRASTRUCTURE ONLY.  Nothing in the product package ``volpick_amd`` may
import this; only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s
``cpu_baseline`` leg use it, as the checker / the timed CPU stand-in.

PARITY UNPINNED.  The arithmetic of the path lives in the un-vendored
third-party packages SeisBench (``seisbench.models``) and ObsPy
(``obspy.signal.trigger.trigger_onset``), which are neither in the
reference repository nor installable here.  The
reference repository holds no tests, golden vectors or fixtures for this path.
This oracle therefore restates the *published* SeisBench (>= 0.4, the
``seisbench_requirement`` in Final_models/**/*.json.v1:8) and ObsPy 1.4
algorithms, anchored on what the reference repository does pin:

  * the released state dicts load with strict key/shape equality
    (Final_models/**/*.pt.v1),
  * forward-call contracts   volpick/model/models.py:157-164,535-549
                             volpick/model/eval_taks0.py:58-142,
  * trigger / peak rule      volpick/model/eval_taks0.py:46-56,
  * stream -> array assembly volpick/data/convert.py:26-70,
  * API usage                README.md:38-82, Final_models/demo.ipynb.

Every constant that the reference does not pin is a named switch in
``oracle.constants`` so that one run on a SeisBench-equipped machine can flip
exactly one value.
"""
