// bdr_local_check.cpp -- a distributed local form (n_owned < ndofs, what ParPAForm builds for a rank)
// has no boundary integrators: PAForm::set_boundary refuses with ERR_UNSUPPORTED and the form stays
// usable.  No C entry point reaches such a form's boundary setters (ParPAForm has no boundary API), so
// this program constructs the C++ class itself; tests/test_gpu_boundary.py builds and runs it.  Needs a
// HIP device (the form's constructor uploads its maps).
#include "pa_form.hpp"

#include <cstdio>
#include <vector>

int main()
{
   using namespace ecm2;
   try
   {
      // one p = 1 element, 8 dofs, the last 4 ghosts
      const std::vector<int> gmap = {0, 1, 2, 3, 4, 5, 6, 7};
      PAForm local(1, 1, 8, gmap.data(), 0, 4);
      PAForm serial(1, 1, 8, gmap.data(), 0, -1);
      const int bmap[4] = {0, 1, 2, 3}, attr[1] = {1};
      const double nodes[12] = {0, 1, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0};
      int code = OK;
      try { local.set_boundary(1, bmap, attr, nodes, 0); }
      catch (const Error &e) { code = e.code; std::printf("refused: %s\n", e.what()); }
      if (code != ERR_UNSUPPORTED) { std::printf("FAIL: code %d, expected %d\n", code, (int)ERR_UNSUPPORTED); return 1; }
      int nbe = -1, ni = -1;
      local.boundary_info(&nbe, &ni, nullptr, nullptr);
      if (nbe != 0 || ni != 0) { std::printf("FAIL: the refused call left boundary data\n"); return 1; }
      serial.set_boundary(1, bmap, attr, nodes, 0);  // the same arguments on a serial form are fine
      serial.boundary_info(&nbe, &ni, nullptr, nullptr);
      if (nbe != 1) { std::printf("FAIL: serial form nbe %d\n", nbe); return 1; }
   }
   catch (const Error &e)
   {
      std::printf("FAIL: %s\n", e.what());
      return 1;
   }
   std::printf("PASS\n");
   return 0;
}
